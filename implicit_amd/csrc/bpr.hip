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
// matrix size (pair_sgd.hip pair_update): Hogwild only works while concurrent samples seldom share a row.  The layout, the
// search, the count reduction, the dispatch over (G, CPL) and the cap live in sgd_group.h, shared with WARP and LMF.
//
// Every id the update kernel turns into an address has been checked on the device first (pair_sgd.hip check_pair_ids): an
// id outside its matrix returns IMP_OUT_OF_RANGE with nothing launched -- an out-of-bounds write is a device fault.
#include "common.h"
#include "philox.h"
#include "sgd_group.h"

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
  const LaneGroup<G> g;
  const int gl = g.gl;
  const int64_t ngroups = g.ngroups;
  const int C = a.C;
  const float lr = a.lr, reg = a.reg;
  unsigned correct = 0, skipped = 0;

  int64_t s = g.index;
  int u = 0, i = 0, j = 0;
  if (s < a.samples) bpr_draw(a, s, u, i, j);
  for (; s < a.samples; s += ngroups) {
    // the next sample's draw and ids do not depend on this one: their loads are in flight while this sample runs
    int un = 0, in = 0, jn = 0;
    if (s + ngroups < a.samples) bpr_draw(a, s + ngroups, un, in, jn);

    // the negative check (sgd_group.h): is j in row u of the pattern
    const bool skip = a.verify && group_row_contains<G>(a.itemids, a.indptr[u], a.indptr[u + 1], j, gl, g.gmask);

    if (skip) {
      skipped += gl == 0;
    } else {
      float *xr = a.X + (size_t)u * C, *yi = a.Y + (size_t)i * C, *yj = a.Y + (size_t)j * C;
      float x[CPL], p[CPL], q[CPL];
      float part = 0.f;
#pragma unroll
      for (int k = 0; k < CPL; ++k) {  // the three rows column by column: not three group_loads, which would reorder the loads
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

}  // namespace imp

using namespace imp;

extern "C" int imp_bpr_update(const imp_intvector *userids, const imp_intvector *itemids, const imp_intvector *indptr, imp_matrix *X,
                              imp_matrix *Y, float learning_rate, float regularization, int64_t seed, int verify_negative,
                              int64_t samples, int64_t *correct, int64_t *skipped) {
  return guarded([&] {
    pair_update("bpr_update", "bpr_check_ids", "bpr_update", userids, itemids, indptr, X, Y, samples, correct, skipped,
                [&](int G, int grid, int64_t n, unsigned long long *stats) {
                  const BprArgs a{userids->v.data(), itemids->v.data(), indptr->v.data(), X->mut<float>(), Y->mut<float>(), (int64_t)userids->size, n,
                                  (uint64_t)seed, learning_rate, regularization, (int)X->cols, verify_negative ? 1 : 0, stats};
                  for_group_shape<false>(G, a.C, [&](auto g, auto cpl) {
                    bpr_update_kernel<decltype(g)::value, decltype(cpl)::value><<<grid, 256, 0, stream()>>>(a);
                  });
                });
  });
}

