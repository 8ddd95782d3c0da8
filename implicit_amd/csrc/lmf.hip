// K10: Logistic Matrix Factorization -- one Adagrad half-sweep of X against a read-only Y (imp_lmf_update).
//
// The reference has no GPU LMF (implicit/lmf.py raises NotImplementedError for use_gpu=True).  The numerical contract is
// its CPU update, implicit/cpu/lmf.pyx lmf_update and fit.  X (rows x C) and Y (other x C), fp32, C = factors + 2; the
// item matrix holds 1.0 in column C-1 (so a user's column C-1 is the user bias), the user matrix 1.0 in column C-2 (so an
// item's column C-2 is the item bias).  `cui` is the CSR of rows of X x rows of Y, values = confidences c.  For every row u
// with n = deg(u) > 0, every dot product taken from the OLD X[u]:
//   d    = sum_p c_p (1 - sigma(X[u].Y[i_p])) Y[i_p]  -  sum_{k<K} sigma(X[u].Y[j_k]) Y[j_k]  -  reg X[u]
//   G[u] += d*d                                      (fp32, as the reference)
//   X[u] += lr / sqrt(1e-6 + G[u]) * d               (element-wise; the step in double, as lmf.pyx's `1e-6 + float` is)
// sigma is the overflow-safe logistic function of lmf.pyx; 1 - sigma(s) is taken as sigma(-s).  Rows with n = 0 are not
// touched (X and G).  After the whole half-sweep column `one_col` of X is 1.0 in EVERY row, empty rows included (one_col
// = C-2 for the user half, C-1 for the item half, -1 for none).
//
// Negatives.  K = min(C, n * neg_prop): the reference caps the count with item_vectors.shape[1] -- the COLUMN count, not
// the number of items -- and this keeps that quirk so that a GPU model trains like stock implicit.  Negative k of row r is
// j = indices[pos] of the CSR being swept, pos uniform over [0, nnz) (popularity-weighted, not checked against the row's
// positives): pos = (w * nnz) >> 32 in 64-bit arithmetic, w = word (k mod 4) of Philox4x32-10 at counter (k / 4, r, 0, 3),
// key (seed_lo, seed_hi) (philox.h).  The negatives, and so the result, are a pure function of (seed, CSR, X, Y); there
// are no float atomics and every sum runs in a fixed order, so two identical calls give bitwise identical X and G.
//
// Layout (sgd_group.h, shared with bpr.hip and warp.hip).  One GROUP of G = 16 / 32 / 64 lanes per row (group_lanes); lane l
// owns columns l, l + G, ... of X[u], the gathered Y rows and the accumulator d.  Row stride is C x 4 bytes (4-byte aligned
// only in general: C = 5, 34, 102), so the loads are dwords, coalesced across the group.  The row's entries -- positives,
// then negatives -- are taken G at a time: lane l first resolves entry l of the chunk to a Y row (indices[p] for a
// positive; the Philox draw and indices[pos] for a negative), all lanes at once; then the group gathers B rows at a time
// (B = 8 / 4 / 2 by row width), so B row loads per group are in flight before the first dot product (a DPP butterfly,
// group_dot) waits.
//
// Row classes (imp_csr): rows of classes 1..6 (1..512 nonzeros) go one group per row, longest first (lmf_rows_kernel).  The
// long rows of class 0 are cut by the CSR's plan_all into segments of <= 512 nonzeros; lmf_segment_kernel writes each
// segment's partial positive sum to a workspace, and lmf_finish_kernel -- one group per long row -- adds the row's
// negatives, then its segments' partials in segment order, and applies Adagrad.
#include <algorithm>

#include "common.h"
#include "philox.h"
#include "sgd_group.h"

namespace imp {

struct LmfArgs {
  const int32_t *__restrict__ indptr;
  const int32_t *__restrict__ indices;
  const float *__restrict__ data;
  const int32_t *__restrict__ order;
  const float *__restrict__ Y;
  float *__restrict__ X;
  float *__restrict__ G;  // Adagrad accumulator, shape of X
  float *__restrict__ ws;  // [n_seg x C] partial sums of the long rows' segments
  LongPlanDev plan;
  int64_t nnz, row_begin, row_end;  // lmf_rows_kernel: order[row_begin .. row_end)
  uint64_t seed;
  float lr, reg;
  int C, neg_prop;
};

__device__ __forceinline__ float lmf_sigmoid(float v) {
  if (v >= 0.f) return 1.f / (1.f + expf(-v));
  const float z = expf(v);
  return z / (1.f + z);
}

__device__ __forceinline__ int lmf_negatives(const LmfArgs &a, int64_t n) {
  return (int)std::min<int64_t>(a.C, n * (int64_t)a.neg_prop);
}

// acc += the positive terms of entries [pbeg, pbeg + n) and the K negative terms of row `row`, dot products with x
template <int G, int CPL, int B>
__device__ __forceinline__ void lmf_accumulate(const LmfArgs &a, int row, const float (&x)[CPL], float (&acc)[CPL], int64_t pbeg,
                                               int n, int K) {
  const int lane = threadIdx.x & 63, gl = lane & (G - 1), gbase = lane & ~(G - 1);
  const int C = a.C;
  const int E = n + K;
  for (int e0 = 0; e0 < E; e0 += G) {  // group-uniform trip count
    // 1. lane gl resolves entry e0 + gl to a Y row: col = -1 past the end, kind 1 positive (weight c), kind 2 negative
    const int e = e0 + gl;
    int col = -1, kind = 0;
    float w = 0.f;
    if (e < n) {
      col = a.indices[pbeg + e];
      w = a.data[pbeg + e];
      kind = 1;
    } else if (e < E) {
      const int k = e - n;
      const u32x4 r = philox4x32_10((uint32_t)(k >> 2), (uint32_t)row, 0u, 3u, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
      const uint32_t word = (k & 3) == 0 ? r.x : (k & 3) == 1 ? r.y : (k & 3) == 2 ? r.z : r.w;
      const int64_t pos = (int64_t)(((uint64_t)word * (uint64_t)a.nnz) >> 32);
      col = a.indices[pos];
      kind = 2;
    }
    // 2. B gathered rows at a time: all B loads issued before the first dot product
    const int chunk = E - e0 < G ? E - e0 : G;
    for (int b0 = 0; b0 < chunk; b0 += B) {
      float y[B][CPL];
      int kb[B];
      float wb[B];
#pragma unroll
      for (int b = 0; b < B; ++b) {
        const int src = gbase + ((b0 + b) & (G - 1));
        const bool live = b0 + b < chunk;
        const int cb = live ? __shfl(col, src) : -1;
        kb[b] = live ? __shfl(kind, src) : 0;
        wb[b] = __shfl(w, src);
        const float *yr = a.Y + (size_t)(cb < 0 ? 0 : cb) * C;
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
          const int c = gl + G * k;
          y[b][k] = (cb >= 0 && c < C) ? yr[c] : 0.f;
        }
      }
#pragma unroll
      for (int b = 0; b < B; ++b) {
        const float s = group_dot<G>(x, y[b]);  // bitwise the same in every lane of the group
        const float coef = kb[b] == 1 ? wb[b] * lmf_sigmoid(-s) : kb[b] == 2 ? -lmf_sigmoid(s) : 0.f;
#pragma unroll
        for (int k = 0; k < CPL; ++k) acc[k] = fmaf(coef, y[b][k], acc[k]);
      }
    }
  }
}

// x = row `row` of X, acc = 0
template <int G, int CPL>
__device__ __forceinline__ void lmf_begin_row(const LmfArgs &a, int gl, int row, float (&x)[CPL], float (&acc)[CPL]) {
  group_load<G>(a.X + (size_t)row * a.C, a.C, gl, x);
#pragma unroll
  for (int k = 0; k < CPL; ++k) acc[k] = 0.f;
}

// d = acc - reg x;  G += d*d;  X += lr / sqrt(1e-6 + G) * d
template <int G, int CPL>
__device__ __forceinline__ void lmf_adagrad(const LmfArgs &a, int gl, int row, const float (&x)[CPL], const float (&acc)[CPL]) {
  float *xr = a.X + (size_t)row * a.C, *gr = a.G + (size_t)row * a.C;
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const int c = gl + G * k;
    if (c < a.C) {
      const float d = acc[k] - a.reg * x[k];
      const float g = gr[c] + d * d;
      gr[c] = g;
      xr[c] = (float)((double)x[k] + (double)a.lr / sqrt(1e-6 + (double)g) * (double)d);
    }
  }
}

template <int CPL> constexpr int lmf_batch() { return CPL <= 2 ? 8 : CPL <= 4 ? 4 : 2; }

// rows of 1 .. 512 nonzeros: order[row_begin .. row_end), one group per row
template <int G, int CPL>
__global__ __launch_bounds__(256) void lmf_rows_kernel(LmfArgs a) {
  const LaneGroup<G> g;
  for (int64_t i = a.row_begin + g.index; i < a.row_end; i += g.ngroups) {
    const int row = a.order[i];
    const int64_t beg = a.indptr[row];
    const int n = a.indptr[row + 1] - (int32_t)beg;
    float x[CPL], acc[CPL];
    lmf_begin_row<G>(a, g.gl, row, x, acc);
    lmf_accumulate<G, CPL, lmf_batch<CPL>()>(a, row, x, acc, beg, n, lmf_negatives(a, n));
    lmf_adagrad<G>(a, g.gl, row, x, acc);
  }
}

// segments of the long rows: the positive terms of seg_begin .. seg_end, to ws[s * C ..]
template <int G, int CPL>
__global__ __launch_bounds__(256) void lmf_segment_kernel(LmfArgs a) {
  const LaneGroup<G> g;
  for (int64_t s = g.index; s < a.plan.n_seg; s += g.ngroups) {
    const int row = a.plan.rows[a.plan.seg_row[s]];
    const int beg = a.plan.seg_begin[s];
    float x[CPL], acc[CPL];
    lmf_begin_row<G>(a, g.gl, row, x, acc);
    lmf_accumulate<G, CPL, lmf_batch<CPL>()>(a, row, x, acc, beg, a.plan.seg_end[s] - beg, 0);
    group_store<G>(a.ws + (size_t)s * a.C, a.C, g.gl, acc);
  }
}

// long rows: negatives, then the segments' partials in segment order, then Adagrad
template <int G, int CPL>
__global__ __launch_bounds__(256) void lmf_finish_kernel(LmfArgs a) {
  const LaneGroup<G> g;
  const int gl = g.gl;
  for (int64_t li = g.index; li < a.plan.n_long; li += g.ngroups) {
    const int row = a.plan.rows[li];
    const int n = a.indptr[row + 1] - a.indptr[row];
    float x[CPL], acc[CPL];
    lmf_begin_row<G>(a, gl, row, x, acc);
    lmf_accumulate<G, CPL, lmf_batch<CPL>()>(a, row, x, acc, 0, 0, lmf_negatives(a, n));
    for (int s = a.plan.row_seg[li]; s < a.plan.row_seg[li + 1]; ++s) {
      const float *p = a.ws + (size_t)s * a.C;
#pragma unroll
      for (int k = 0; k < CPL; ++k)
        if (gl + G * k < a.C) acc[k] += p[gl + G * k];
    }
    lmf_adagrad<G>(a, gl, row, x, acc);
  }
}

__global__ __launch_bounds__(256) void lmf_one_col_kernel(float *X, int64_t rows, int C, int one_col) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x)
    X[(size_t)r * C + one_col] = 1.f;
}

enum LmfPass { kLmfRows, kLmfSegments, kLmfFinish };

template <int G, int CPL> static void launch_lmf_pass(const LmfArgs &a, LmfPass pass, int grid) {
  if (pass == kLmfRows) lmf_rows_kernel<G, CPL><<<grid, 256, 0, stream()>>>(a);
  else if (pass == kLmfSegments) lmf_segment_kernel<G, CPL><<<grid, 256, 0, stream()>>>(a);
  else lmf_finish_kernel<G, CPL><<<grid, 256, 0, stream()>>>(a);
}

// G by the rule alone (sgd_group.h group_lanes; IMP_BPR_LANES is not read here), so the 12 (G, CPL) it reaches are compiled
static void launch_lmf(const LmfArgs &a, LmfPass pass, int64_t work) {
  const int G = group_lanes(a.C);
  const int grid = (int)std::min<int64_t>((work * G + 255) / 256, (int64_t)ctx().num_cus * 8);
  for_group_shape<true>(G, a.C, [&](auto g, auto cpl) { launch_lmf_pass<decltype(g)::value, decltype(cpl)::value>(a, pass, grid); });
  IMP_CHECK_HIP(hipGetLastError());
}

}  // namespace imp

using namespace imp;

extern "C" int imp_lmf_update(const imp_csr *cui, imp_matrix *X, const imp_matrix *Y, imp_matrix *deriv_sum_sq, float learning_rate,
                              float regularization, int neg_prop, int64_t seed, int one_col) {
  return guarded([&] {
    if (!cui || !X || !Y || !deriv_sum_sq) throw std::invalid_argument("lmf_update: NULL argument");
    if ((int64_t)X->rows != cui->rows) throw std::invalid_argument("lmf_update: X.rows must equal the CSR's rows");
    if ((int64_t)Y->rows != cui->cols) throw std::invalid_argument("lmf_update: Y.rows must equal the CSR's columns");
    if (X->cols != Y->cols) throw std::invalid_argument("X and Y should have the same number of columns");
    if (deriv_sum_sq->rows != X->rows || deriv_sum_sq->cols != X->cols)
      throw std::invalid_argument("lmf_update: deriv_sum_sq must have the shape of X");
    if (X->itemsize != 4 || Y->itemsize != 4 || deriv_sum_sq->itemsize != 4)
      throw std::invalid_argument("lmf_update: X, Y and deriv_sum_sq must be float32");
    if (X->cols < 3 || X->cols > 1024)
      throw std::invalid_argument("lmf_update: factor matrices need 3 .. 1024 columns (factors + 2 for the biases)");
    const int C = (int)X->cols;
    if (neg_prop < 0) throw std::invalid_argument("lmf_update: neg_prop must be >= 0");
    if (one_col < -1 || one_col >= C) throw std::invalid_argument("lmf_update: one_col must lie in [-1, C)");
    if (X->overlaps(Y) || X->overlaps(deriv_sum_sq) || deriv_sum_sq->overlaps(Y))
      throw std::invalid_argument("lmf_update: X, Y and deriv_sum_sq must not share storage");
    if (!cui->parts.empty())
      throw std::invalid_argument("lmf_update: a CSR held in several >2^31-nonzero blocks is not supported");

    float *const x = X->mut<float>();  // (cached top-k planes made from X are stale from here on)
    if (cui->nnz > 0) {
      const LongPlan &lp = cui->plan_all;
      LmfArgs a{cui->indptr.data(), cui->indices.data(), cui->data.data(), cui->order.data(), Y->f32(), x, deriv_sum_sq->mut<float>(),
                nullptr, lp.dev(cui->order.data()), cui->nnz, cui->bin_start[1], cui->bin_start[imp_csr::kBins - 1], (uint64_t)seed,
                learning_rate, regularization, C, neg_prop};
      if (lp.n_seg > 0) {
        a.ws = ctx().lmf_ws.reserve((size_t)lp.n_seg * C);
        IMP_PROF("lmf_segments");
        launch_lmf(a, kLmfSegments, lp.n_seg);
      }
      if (a.row_end > a.row_begin) {
        IMP_PROF("lmf_rows");
        launch_lmf(a, kLmfRows, a.row_end - a.row_begin);
      }
      if (lp.n_long > 0) {
        IMP_PROF("lmf_finish");
        launch_lmf(a, kLmfFinish, lp.n_long);
      }
    }
    if (one_col >= 0 && X->rows > 0) {
      const int grid = (int)std::min<int64_t>(((int64_t)X->rows + 255) / 256, (int64_t)ctx().num_cus * 4);
      lmf_one_col_kernel<<<grid, 256, 0, stream()>>>(x, (int64_t)X->rows, C, one_col);
      IMP_CHECK_HIP(hipGetLastError());
    }
    sync();  // synchronous, deferred mode included
  });
}
