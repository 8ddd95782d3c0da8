// K9: Bayesian Personalized Ranking -- one SGD epoch over sampled (user, liked, disliked) triples (imp_bpr_update).
//
// Replaces implicit/gpu/bpr.cu:16-125 (reference).  The numerical contract is the reference's CPU update,
// implicit/cpu/bpr.pyx:249-302, not the CUDA kernel.  With X (users x C) and Y (items x C), C = factors + 1, and column
// C-1 the bias column (1.0 in every user row), one sample is:
//   1. lp, dp uniform over [0, nnz) (below); u = userids[lp], i = itemids[lp], j = itemids[dp] -- negatives are drawn by
//      popularity, as in both reference paths;
//   2. verify_negative and j in row u of the CSR pattern (row indices sorted): counted as skipped, nothing written;
//   3. score = sum_{c < C} X[u,c] (Y[i,c] - Y[j,c]),  z = 1 / (1 + exp(score));  counted as correct when z < 0.5;
//   4. for c < C-1, all from the values before the update:
//        X[u,c] += lr (z (Y[i,c] - Y[j,c]) - reg X[u,c])
//        Y[i,c] += lr (z X[u,c] - reg Y[i,c])
//        Y[j,c] += lr (-z X[u,c] - reg Y[j,c])
//   5. bias column: Y[i,C-1] += lr (z - reg Y[i,C-1]),  Y[j,C-1] += lr (-z - reg Y[j,C-1]);  X[u,C-1] is never written
//      (bpr.cu:60,114 does write it: its `factors` is X->cols);
//   6. i == j (only possible without verification): the j update applies to the value the i update produced, as the
//      serial CPU loop does.
// Sampling: sample s of a call draws r = Philox4x32-10(counter (s_lo, s_hi, 0, 2), key (seed_lo, seed_hi)) (philox.h)
// and takes lp = (r.x * nnz) >> 32, dp = (r.y * nnz) >> 32 in 64-bit arithmetic: the sample set -- and so the skipped
// count -- is a pure function of (seed, s, nnz).  Concurrent samples update shared rows without atomics ("Hogwild", as
// both reference paths), so the factors of a multi-sample call are not bitwise reproducible; the counts are.
//
// Layout: one GROUP of G = 16 / 32 / 64 lanes per sample (wave64 holds 64 / G samples at once).  Lane l of a group owns
// columns l, l + G, l + 2G, ... of the three rows, in registers (CPL columns per lane): every load and store of a row is
// coalesced, the dot product is a register butterfly inside the group (wave_ops.h group_allsum), no LDS and no barrier
// on the sample path.  The negative check is a G-ary search: the group's lanes load G splitters of the row, a ballot
// narrows the range to one of G slices -- ceil(log_G(deg)) dependent loads instead of log2(deg).  The ids of a group's
// next sample are loaded while the current one is searched and updated.  The number of samples in flight is capped by the
// matrix size (see the launch): Hogwild only works while concurrent samples seldom share a row.  The search, the count
// reduction, the dispatch over CPL and the cap live in pair_sgd.h, shared with the WARP kernel (warp.hip).
//
// Every id the update kernel turns into an address has been checked on the device first (bpr_check_kernel): an id
// outside its matrix returns IMP_OUT_OF_RANGE with nothing launched -- an out-of-bounds write is a device fault.
#include <cstdlib>

#include "common.h"
#include "pair_sgd.h"
#include "philox.h"
#include "wave_ops.h"

namespace imp {

struct BprArgs {
  const int32_t *__restrict__ userids;
  const int32_t *__restrict__ itemids;
  const int32_t *__restrict__ indptr;
  float *X, *Y;  // may alias each other's rows across samples (Hogwild): no __restrict__
  int64_t nnz, samples;
  uint64_t seed;
  float lr, reg;
  int C, verify;
  unsigned long long *stats;  // [0] correct, [1] skipped
};

__device__ __forceinline__ void bpr_draw(const BprArgs &a, int64_t s, int &u, int &i, int &j) {
  const u32x4 r = philox4x32_10((uint32_t)s, (uint32_t)((uint64_t)s >> 32), 0u, 2u, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
  const int64_t lp = (int64_t)(((uint64_t)r.x * (uint64_t)a.nnz) >> 32);
  const int64_t dp = (int64_t)(((uint64_t)r.y * (uint64_t)a.nnz) >> 32);
  u = a.userids[lp];
  i = a.itemids[lp];
  j = a.itemids[dp];
}

template <int G, int CPL>
__global__ __launch_bounds__(256) void bpr_update_kernel(BprArgs a) {
  const int lane = threadIdx.x & 63;
  const int gl = lane & (G - 1);  // lane inside the group
  const uint64_t gmask = group_mask<G>(lane);
  const int64_t ngroups = (int64_t)gridDim.x * (blockDim.x / G);
  const int C = a.C;
  const float lr = a.lr, reg = a.reg;
  unsigned correct = 0, skipped = 0;

  int64_t s = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
  int u = 0, i = 0, j = 0;
  if (s < a.samples) bpr_draw(a, s, u, i, j);
  for (; s < a.samples; s += ngroups) {
    // the next sample's draw and ids do not depend on this one: their loads are in flight while this sample runs
    int un = 0, in = 0, jn = 0;
    if (s + ngroups < a.samples) bpr_draw(a, s + ngroups, un, in, jn);

    // the negative check (pair_sgd.h): is j in row u of the pattern
    const bool skip = a.verify && group_row_contains<G>(a.itemids, a.indptr[u], a.indptr[u + 1], j, gl, gmask);

    if (skip) {
      skipped += gl == 0;
    } else {
      float *xr = a.X + (size_t)u * C, *yi = a.Y + (size_t)i * C, *yj = a.Y + (size_t)j * C;
      float x[CPL], p[CPL], q[CPL];
      float part = 0.f;
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int c = gl + G * k;
        const bool in_row = c < C;
        x[k] = in_row ? xr[c] : 0.f;
        p[k] = in_row ? yi[c] : 0.f;
        q[k] = in_row ? yj[c] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < CPL; ++k) part = fmaf(x[k], p[k] - q[k], part);
      const float score = group_allsum<G>(part);  // bitwise the same in every lane of the group
      const float z = 1.f / (1.f + expf(score));
      correct += gl == 0 && z < 0.5f;
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int c = gl + G * k;
        if (c < C) {
          const bool bias = c == C - 1;
          const float ni = p[k] + lr * ((bias ? z : z * x[k]) - reg * p[k]);
          const float pj = i == j ? ni : q[k];
          const float nj = pj + lr * ((bias ? -z : -z * x[k]) - reg * pj);
          if (!bias) xr[c] = x[k] + lr * (z * (p[k] - q[k]) - reg * x[k]);
          if (i != j) yi[c] = ni;
          yj[c] = nj;
        }
      }
    }
    u = un, i = in, j = jn;
  }

  block_add_counts(correct, skipped, a.stats);
}

// The pre-pass: 0 <= userids < x_rows, 0 <= itemids < y_rows, 0 <= indptr <= nnz.  Violations OR bits 1 / 2 / 4 into *bad.
// The first `quads` x 4 ids are read as int4 (16-byte aligned arrays), the rest one by one.
__global__ __launch_bounds__(256) void bpr_check_kernel(const int32_t *__restrict__ userids, const int32_t *__restrict__ itemids,
                                                        int64_t nnz, int64_t quads, const int32_t *__restrict__ indptr,
                                                        int64_t n_indptr, int64_t x_rows, int64_t y_rows, unsigned long long *bad) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  unsigned flags = 0;
  auto user_ok = [&](int32_t v) { return v >= 0 && v < x_rows; };
  auto item_ok = [&](int32_t v) { return v >= 0 && v < y_rows; };
  for (int64_t k = tid; k < quads; k += stride) {
    const int4 us = reinterpret_cast<const int4 *>(userids)[k];
    const int4 is = reinterpret_cast<const int4 *>(itemids)[k];
    if (!(user_ok(us.x) && user_ok(us.y) && user_ok(us.z) && user_ok(us.w))) flags |= 1;
    if (!(item_ok(is.x) && item_ok(is.y) && item_ok(is.z) && item_ok(is.w))) flags |= 2;
  }
  for (int64_t k = 4 * quads + tid; k < nnz; k += stride) {
    if (!user_ok(userids[k])) flags |= 1;
    if (!item_ok(itemids[k])) flags |= 2;
  }
  for (int64_t k = tid; k < n_indptr; k += stride) {
    const int32_t v = indptr[k];
    if (v < 0 || v > nnz) flags |= 4;
  }
  if (flags) atomicOr(bad, (unsigned long long)flags);
}

// lanes per sample: the narrowest group that keeps a row in at most 8 registers per lane (more samples per wave in flight),
// IMP_BPR_LANES=16/32/64 overrides it for measurement where C <= 16 x lanes
int bpr_group(int C) {
  if (const char *e = std::getenv("IMP_BPR_LANES")) {
    const int g = std::atoi(e);
    if ((g == 16 || g == 32 || g == 64) && C <= 16 * g) return g;
  }
  return C <= 128 ? 16 : C <= 256 ? 32 : 64;
}

template <int G> static void launch_bpr(const BprArgs &a, int grid) {
  for_columns_per_lane((a.C + G - 1) / G, [&](auto cpl) { bpr_update_kernel<G, decltype(cpl)::value><<<grid, 256, 0, stream()>>>(a); });
}

void check_pair_ids(const char *who, const char *prof, const imp_intvector *userids, const imp_intvector *itemids,
                    const imp_intvector *indptr, size_t x_rows, size_t y_rows, unsigned long long *bad_word) {
  const int64_t nnz = (int64_t)userids->size;
  {
    IMP_PROF(prof);
    const int64_t work = std::max(nnz / 4, (int64_t)indptr->size);
    const int grid = (int)std::min<int64_t>((work + 255) / 256, ctx().num_cus * 8);
    const bool aligned = ((uintptr_t)userids->v.data() | (uintptr_t)itemids->v.data()) % 16 == 0;
    bpr_check_kernel<<<grid, 256, 0, stream()>>>(userids->v.data(), itemids->v.data(), nnz, aligned ? nnz / 4 : 0, indptr->v.data(),
                                                 (int64_t)indptr->size, (int64_t)x_rows, (int64_t)y_rows, bad_word);
    IMP_CHECK_HIP(hipGetLastError());
  }
  unsigned long long bad = 0;
  IMP_CHECK_HIP(hipMemcpyAsync(&bad, bad_word, sizeof(bad), hipMemcpyDeviceToHost, stream()));
  sync();
  const std::string w(who);
  if (bad & 1) throw out_of_range_error(w + ": a user id is outside [0, X.rows)");
  if (bad & 2) throw out_of_range_error(w + ": an item id is outside [0, Y.rows)");
  if (bad & 4) throw out_of_range_error(w + ": an indptr entry is outside [0, nnz]");
}

}  // namespace imp

using namespace imp;

extern "C" int imp_bpr_update(const imp_intvector *userids, const imp_intvector *itemids, const imp_intvector *indptr, imp_matrix *X,
                              imp_matrix *Y, float learning_rate, float regularization, int64_t seed, int verify_negative,
                              int64_t samples, int64_t *correct, int64_t *skipped) {
  return guarded([&] {
    if (!userids || !itemids || !indptr || !X || !Y || !correct || !skipped) throw std::invalid_argument("bpr_update: NULL argument");
    if (X->cols != Y->cols) throw std::invalid_argument("X and Y should have the same number of columns");
    if (X->cols < 2 || X->cols > 1024)
      throw std::invalid_argument("bpr_update: factor matrices need 2 .. 1024 columns (factors + 1 for the item bias)");
    if (X->itemsize != 4 || Y->itemsize != 4) throw std::invalid_argument("bpr_update: factor matrices must be float32");
    if (userids->size != itemids->size) throw std::invalid_argument("userids and itemids should have same number of elements");
    if (indptr->size != X->rows + 1) throw std::invalid_argument("bpr_update: indptr must have X.rows + 1 entries");
    const int64_t nnz = (int64_t)userids->size;
    if (nnz > INT32_MAX) throw std::invalid_argument("bpr_update: more than 2^31 - 1 nonzeros");
    const int64_t n = samples < 0 ? nnz : samples;
    *correct = *skipped = 0;
    if (nnz == 0 || n == 0) return;

    auto &st = ctx().pair_stats;
    if (st.size < 3) st.alloc(3);
    unsigned long long *stats = st.data();
    IMP_CHECK_HIP(hipMemsetAsync(stats, 0, 3 * sizeof(unsigned long long), stream()));
    const int cap = ctx().num_cus * 8;  // 8 workgroups of 4 waves per CU: the most the CU holds
    check_pair_ids("bpr_update", "bpr_check_ids", userids, itemids, indptr, X->rows, Y->rows, stats + 2);

    note_device_write(X->data, X->bytes());  // cached top-k planes and padded copies made from X or Y are stale after this
    note_device_write(Y->data, Y->bytes());
    BprArgs a{userids->v.data(), itemids->v.data(), indptr->v.data(), X->f32(), Y->f32(), nnz, n, (uint64_t)seed,
              learning_rate, regularization, (int)X->cols, verify_negative ? 1 : 0, stats};
    {
      IMP_PROF("bpr_update");
      const int G = bpr_group(a.C);
      const int64_t in_flight = hogwild_in_flight(n, X->rows, Y->rows);  // the cap on concurrent samples: pair_sgd.h
      const int grid = (int)std::min<int64_t>((in_flight * G + 255) / 256, cap);
      if (G == 16) launch_bpr<16>(a, grid);
      else if (G == 32) launch_bpr<32>(a, grid);
      else launch_bpr<64>(a, grid);
      IMP_CHECK_HIP(hipGetLastError());
    }
    unsigned long long h[2];
    IMP_CHECK_HIP(hipMemcpyAsync(h, stats, sizeof(h), hipMemcpyDeviceToHost, stream()));
    sync();  // synchronous in deferred mode too: the counts are the result
    *correct = (int64_t)h[0];
    *skipped = (int64_t)h[1];
  });
}
