// K18: the two products of the randomized SVD: imp_csr_spmm, imp_matrix_multiply_small.  No floating-point
// atomics: equal inputs give bitwise equal outputs.
//
// imp_csr_spmm   out = A D, every entry the chain ((0 + a_1 D[j_1][c]) + a_2 D[j_2][c]) + ... over the row's stored entries,
//   products and sums rounded separately.  Three kernels, every dependency a kernel boundary (the shape of als_subspace.hip):
//   spmm_wave_kernel     rows of <= kCholLongRow nonzeros, longest first from the schedule, l > 32: a wavefront owns a destination
//     row and a slab of 64 NQ columns, lane t the columns t, t + 64, ...; it reads 64 (column, value) pairs of the row at a time,
//     one per lane, and broadcasts them from there, gathering four source rows of D before it adds them in stored order.
//   spmm_group_kernel    the same rows for l <= 32: P = the power of two >= l lanes own a row, 64 / P rows share a wavefront.
//   spmm_partial_kernel  rows of more nonzeros: a wavefront per (segment of plan_chol, slab), the same chain from 0 into a
//     workspace; spmm_fold_kernel then adds a row's partials in segment order, starting from the first segment's.
//   Empty rows are zeroed by zero_rows.
// imp_matrix_multiply_small   out = Y W on 128 x 128 x 16 tiles, both operands staged through the LDS, 2 x 2 tiles of
//   v_mfma_f32_32x32x2_f32 per wavefront (the building block of spd_inverse.hip with B not transposed): exact fp32 products,
//   sums over k in ascending order.
#include <algorithm>

#include "common.h"

namespace imp {

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {
constexpr int kSpmmMaxCols = 1024;  // of D and out; of both operands of multiply_small
constexpr int kSpmmMaxNQ = 8;       // columns a lane owns in spmm_wave_kernel / spmm_partial_kernel
constexpr int kSpmmGroupCols = 32;  // l up to here: several rows per wavefront

__device__ __forceinline__ float lane_value(float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }

// s[q] = (s[q] + a_p D[j_p][c[q]]) for the nonzeros p in [rb, re) in stored order; rb, re are wave-uniform
template <int NQ>
__device__ __forceinline__ void spmm_chain(const int32_t *__restrict__ indices, const float *__restrict__ data,
                                           const float *__restrict__ D, int l, long rb, long re, const int (&c)[NQ], float (&s)[NQ],
                                           int lane) {
  for (long pb = rb; pb < re; pb += 64) {
    const int cnt = (int)min(64L, re - pb);
    int jv = 0;
    float av = 0.f;
    if (lane < cnt) jv = indices[pb + lane], av = data[pb + lane];
    int e = 0;
    for (; e + 4 <= cnt; e += 4) {  // four source rows in flight
      float a[4], d[4][NQ];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float *row = D + (size_t)__builtin_amdgcn_readlane(jv, e + u) * l;
        a[u] = lane_value(av, e + u);
#pragma unroll
        for (int q = 0; q < NQ; ++q) d[u][q] = row[c[q]];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int q = 0; q < NQ; ++q) s[q] = s[q] + a[u] * d[u][q];
    }
    for (; e < cnt; ++e) {
      const float *row = D + (size_t)__builtin_amdgcn_readlane(jv, e) * l;
      const float a = lane_value(av, e);
#pragma unroll
      for (int q = 0; q < NQ; ++q) s[q] = s[q] + a * row[c[q]];
    }
  }
}

// the columns of slab blockIdx.y a lane owns; one past the matrix reads the last column and is never stored
template <int NQ> __device__ __forceinline__ void spmm_columns(int l, int lane, int (&col)[NQ], int (&c)[NQ], float (&s)[NQ]) {
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    col[q] = (int)blockIdx.y * 64 * NQ + 64 * q + lane;
    c[q] = min(col[q], l - 1);
    s[q] = 0.f;
  }
}

template <int NQ>
__global__ __launch_bounds__(256) void spmm_wave_kernel(const int32_t *__restrict__ order, int first, int count,
                                                        const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                        const float *__restrict__ data, const float *__restrict__ D, int l,
                                                        float *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
  const int nwaves = (gridDim.x * blockDim.x) >> 6;
  for (int ri = wave; ri < count; ri += nwaves) {
    const int r = __builtin_amdgcn_readfirstlane(order[first + ri]);
    const int rb = __builtin_amdgcn_readfirstlane(indptr[r]), re = __builtin_amdgcn_readfirstlane(indptr[r + 1]);
    int col[NQ], c[NQ];
    float s[NQ];
    spmm_columns<NQ>(l, lane, col, c, s);
    spmm_chain<NQ>(indices, data, D, l, rb, re, c, s, lane);
    float *dst = out + (size_t)r * l;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      if (col[q] < l) dst[col[q]] = s[q];
  }
}

// l <= 32: lane group g of 1 << shift lanes owns row order[first + g], its lane t column t
__global__ __launch_bounds__(256) void spmm_group_kernel(const int32_t *__restrict__ order, int first, int count,
                                                         const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                         const float *__restrict__ data, const float *__restrict__ D, int l, int shift,
                                                         float *__restrict__ out) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long ri = t >> shift;
  const int col = (int)(t & ((1 << shift) - 1));
  if (ri >= count || col >= l) return;
  const int r = order[first + ri];
  const int rb = indptr[r], re = indptr[r + 1];
  float s = 0.f;
  int p = rb;
  for (; p + 4 <= re; p += 4) {
    float a[4], d[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) a[u] = data[p + u], d[u] = D[(size_t)indices[p + u] * l + col];
#pragma unroll
    for (int u = 0; u < 4; ++u) s = s + a[u] * d[u];
  }
  for (; p < re; ++p) s = s + data[p] * D[(size_t)indices[p] * l + col];
  out[(size_t)r * l + col] = s;
}

// one wavefront per (segment, slab): the segment's chain from 0 into partials[segment][column]
template <int NQ>
__global__ __launch_bounds__(256) void spmm_partial_kernel(const LongPlanDev plan, const int32_t *__restrict__ indices,
                                                           const float *__restrict__ data, const float *__restrict__ D, int l,
                                                           float *__restrict__ partials) {
  const int lane = threadIdx.x & 63;
  const int sg = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
  if (sg >= plan.n_seg) return;
  const int rb = __builtin_amdgcn_readfirstlane(plan.seg_begin[sg]), re = __builtin_amdgcn_readfirstlane(plan.seg_end[sg]);
  int col[NQ], c[NQ];
  float s[NQ];
  spmm_columns<NQ>(l, lane, col, c, s);
  spmm_chain<NQ>(indices, data, D, l, rb, re, c, s, lane);
  float *dst = partials + (size_t)sg * l;
#pragma unroll
  for (int q = 0; q < NQ; ++q)
    if (col[q] < l) dst[col[q]] = s[q];
}

// thread (long row, column): the row's partials added in segment order, starting from the first segment's
__global__ __launch_bounds__(256) void spmm_fold_kernel(const LongPlanDev plan, const float *__restrict__ partials, int l,
                                                        float *__restrict__ out) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long li = t / l;
  const int col = (int)(t - li * l);
  if (li >= plan.n_long) return;
  const int s0 = plan.row_seg[li], s1 = plan.row_seg[li + 1];
  float s = partials[(size_t)s0 * l + col];
  for (int sg = s0 + 1; sg < s1; ++sg) s = s + partials[(size_t)sg * l + col];
  out[(size_t)plan.rows[li] * l + col] = s;
}

// the rows of more than kCholLongRow nonzeros: partials, then the fold
template <int NQ> void spmm_long_rows(const imp_csr *A, const LongPlanDev &plan, const float *D, int l, int slabs, float *out) {
  if (plan.n_seg == 0) return;
  DeviceArray<float> ws;  // the segments' partials; the block outlives the kernels queued here (Storage)
  float *partials = ws.reserve((size_t)plan.n_seg * l);
  IMP_PROF("spmm_long_rows");
  spmm_partial_kernel<NQ><<<dim3((unsigned)((plan.n_seg + 3) / 4), (unsigned)slabs), 256, 0, stream()>>>(
      plan, A->indices.data(), A->data.data(), D, l, partials);
  IMP_CHECK_HIP(hipGetLastError());
  spmm_fold_kernel<<<(unsigned)(((size_t)plan.n_long * l + 255) / 256), 256, 0, stream()>>>(plan, partials, l, out);
  IMP_CHECK_HIP(hipGetLastError());
}

template <int NQ> void spmm_wide(const imp_csr *A, const LongPlanDev &plan, const float *D, int l, int slabs, float *out) {
  spmm_long_rows<NQ>(A, plan, D, l, slabs, out);
  const int n_wave = A->nonempty() - plan.n_long;
  if (n_wave == 0) return;
  IMP_PROF("spmm_wave_rows");
  const int grid = std::min((n_wave + 3) / 4, ctx().num_cus * 16);
  spmm_wave_kernel<NQ><<<dim3((unsigned)grid, (unsigned)slabs), 256, 0, stream()>>>(
      A->order.data(), plan.n_long, n_wave, A->indptr.data(), A->indices.data(), A->data.data(), D, l, out);
  IMP_CHECK_HIP(hipGetLastError());
}

void spmm_narrow(const imp_csr *A, const LongPlanDev &plan, const float *D, int l, float *out) {
  spmm_long_rows<1>(A, plan, D, l, 1, out);
  const int n_group = A->nonempty() - plan.n_long;
  if (n_group == 0) return;
  IMP_PROF("spmm_group_rows");
  int shift = 0;
  while ((1 << shift) < l) ++shift;
  const size_t threads = (size_t)n_group << shift;
  spmm_group_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, stream()>>>(A->order.data(), plan.n_long, n_group, A->indptr.data(),
                                                                            A->indices.data(), A->data.data(), D, l, shift, out);
  IMP_CHECK_HIP(hipGetLastError());
}

void spmm_launch(const imp_csr *A, const float *D, int l, float *out) {
  const LongPlanDev plan = A->plan_chol.dev(A->order.data());
  if (l <= kSpmmGroupCols) {
    spmm_narrow(A, plan, D, l, out);
  } else {
    // 64-column chunks dealt evenly to as few slabs as kSpmmMaxNQ chunks per lane allow
    const int chunks = (l + 63) / 64, slabs = (chunks + kSpmmMaxNQ - 1) / kSpmmMaxNQ, nq = (chunks + slabs - 1) / slabs;
    switch (nq) {
      case 1: spmm_wide<1>(A, plan, D, l, slabs, out); break;
      case 2: spmm_wide<2>(A, plan, D, l, slabs, out); break;
      case 3: spmm_wide<3>(A, plan, D, l, slabs, out); break;
      case 4: spmm_wide<4>(A, plan, D, l, slabs, out); break;
      case 5: spmm_wide<5>(A, plan, D, l, slabs, out); break;
      case 6: spmm_wide<6>(A, plan, D, l, slabs, out); break;
      case 7: spmm_wide<7>(A, plan, D, l, slabs, out); break;
      default: spmm_wide<8>(A, plan, D, l, slabs, out); break;
    }
  }
  zero_rows(A->order.data(), A->first_empty(), A->n_empty(), out, l);
}

// ---- out = Y W ---------------------------------------------------------------------------------------------------------------
constexpr int kMulTile = 128, kMulK = 16, kMulLd = kMulK + 1;

__global__ __launch_bounds__(256) void multiply_small_kernel(const float *__restrict__ Y, long rows, int l, const float *__restrict__ W,
                                                             int m, float *__restrict__ out) {
  __shared__ float As[kMulTile * kMulLd], Bs[kMulTile * kMulLd];  // [row of Y][k] and [column of W][k]
  const long row0 = (long)blockIdx.x * kMulTile;
  const int col0 = blockIdx.y * kMulTile;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int kcol = tid & 15, rbase = tid >> 4;  // Y: 16 consecutive k of a row per 16 threads
  const int wcol = tid & 127, wk = tid >> 7;    // W: 128 consecutive columns of a row of W per 128 threads
  float ra[8], rb[8];
  auto fetch = [&](int kk) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const long r = row0 + rbase + 16 * i;
      ra[i] = (kk + kcol < l && r < rows) ? Y[r * l + kk + kcol] : 0.f;
      const int k = kk + wk + 2 * i;
      rb[i] = (k < l && col0 + wcol < m) ? W[(long)k * m + col0 + wcol] : 0.f;
    }
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 2; ++nj)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[mi][nj][e] = 0.f;
  fetch(0);
  const int a_off = (wm * 64 + (lane & 31)) * kMulLd + (lane >> 5);
  const int b_off = (wn * 64 + (lane & 31)) * kMulLd + (lane >> 5);
  for (int k = 0; k < l; k += kMulK) {
    __syncthreads();  // the previous chunk has been consumed
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      As[(rbase + 16 * i) * kMulLd + kcol] = ra[i];
      Bs[wcol * kMulLd + wk + 2 * i] = rb[i];
    }
    __syncthreads();
    if (k + kMulK < l) fetch(k + kMulK);  // in flight during the products below
#pragma unroll
    for (int ks = 0; ks < kMulK / 2; ++ks) {
      const float a0 = As[a_off + 2 * ks], a1 = As[a_off + 32 * kMulLd + 2 * ks];
      const float b0 = Bs[b_off + 2 * ks], b1 = Bs[b_off + 32 * kMulLd + 2 * ks];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
  // C/D layout of a 32 x 32 tile: col = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 2; ++nj) {
      const int c = col0 + wn * 64 + nj * 32 + (lane & 31);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const long r = row0 + wm * 64 + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        if (r < rows && c < m) out[r * m + c] = acc[mi][nj][e];
      }
    }
}
}  // namespace

}  // namespace imp

using namespace imp;

extern "C" int imp_csr_spmm(const imp_csr *A, const imp_matrix *D, imp_matrix *out) {
  return guarded([&] {
    if (!A || !D || !out) throw std::invalid_argument("csr_spmm: NULL argument");
    if (!A->parts.empty() || A->nnz > INT32_MAX) throw std::invalid_argument("csr_spmm: more than 2^31-1 nonzeros is not supported");
    if (D->itemsize != 4 || out->itemsize != 4) throw std::invalid_argument("csr_spmm: D and out must be float32");
    if (D->cols < 1 || D->cols > (size_t)kSpmmMaxCols)
      throw std::invalid_argument("csr_spmm: D must have 1 .. " + std::to_string(kSpmmMaxCols) + " columns");
    if (D->rows != (size_t)A->cols || out->rows != (size_t)A->rows || out->cols != D->cols)
      throw std::invalid_argument("csr_spmm: A (rows x cols), D (cols x l) and out (rows x l) do not agree");
    if (out->overlaps(D)) throw std::invalid_argument("csr_spmm: out must not share storage with D");
    if (A->rows == 0) return;
    spmm_launch(A, D->f32(), (int)D->cols, out->mut<float>());
    sync_call();
  });
}

extern "C" int imp_matrix_multiply_small(const imp_matrix *Y, const imp_matrix *W, imp_matrix *out) {
  return guarded([&] {
    if (!Y || !W || !out) throw std::invalid_argument("matrix_multiply_small: NULL argument");
    if (Y->itemsize != 4 || W->itemsize != 4 || out->itemsize != 4)
      throw std::invalid_argument("matrix_multiply_small: Y, W and out must be float32");
    if (W->rows < 1 || W->rows > (size_t)kSpmmMaxCols || W->cols < 1 || W->cols > (size_t)kSpmmMaxCols)
      throw std::invalid_argument("matrix_multiply_small: W must be l x m with l and m in 1 .. " + std::to_string(kSpmmMaxCols));
    if (Y->cols != W->rows || out->rows != Y->rows || out->cols != W->cols)
      throw std::invalid_argument("matrix_multiply_small: Y (rows x l), W (l x m) and out (rows x m) do not agree");
    if (out->overlaps(Y) || out->overlaps(W)) throw std::invalid_argument("matrix_multiply_small: out must not share storage with Y or W");
    if (Y->rows == 0) return;
    const size_t row_tiles = (Y->rows + kMulTile - 1) / kMulTile;
    IMP_PROF("multiply_small");
    const int l = (int)W->rows, m = (int)W->cols;
    multiply_small_kernel<<<dim3((unsigned)row_tiles, (unsigned)((m + kMulTile - 1) / kMulTile)), 256, 0, stream()>>>(
        Y->f32(), (long)Y->rows, l, W->f32(), m, out->mut<float>());
    IMP_CHECK_HIP(hipGetLastError());
    sync_call();
  });
}
