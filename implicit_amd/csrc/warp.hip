// K15: WARP-loss matrix factorization -- one SGD epoch over sampled positives, each against uniformly drawn negatives
// until one violates the margin (imp_warp_update).
//
// No reference counterpart: the loss is Weston, Bengio and Usunier, "WSABIE: Scaling Up To Large Vocabulary Image
// Annotation" (IJCAI 2011).  X (users x C) and Y (items x C) are float32 with C = factors + 1, 2 <= C <= 1024; column C-1 is
// the item bias, 1.0 in every user row and never written in X (as in bpr.hip).  userids / itemids are the COO ids of the
// CSR pattern, indptr its row pointers, row indices sorted; nnz < 2^31, items = Y.rows.  Sample s of a call, 0 <= s < samples:
//   1. r = Philox4x32-10(counter (s_lo, s_hi, 0, 4), key (seed_lo, seed_hi)) (philox.h);  lp = (r.x * nnz) >> 32 in 64-bit
//      arithmetic;  u = userids[lp], i = itemids[lp];
//   2. sp = sum_{c < C} X[u,c] Y[i,c];
//   3. trials t = 1 .. max_sampled (1 <= max_sampled <= 4096): word (t-1) & 3 of Philox(counter (s_lo, s_hi,
//      1 + ((t-1) >> 2), 4), same key) gives j = (word * items) >> 32 -- uniform over the items, not by popularity.  j in row
//      u of the pattern: the trial is consumed, nothing else happens.  Otherwise sn = sum_c X[u,c] Y[j,c] and the trial
//      VIOLATES when sn > sp - 1;
//   4. on the first violating trial t:  L = min(10, log(max(1, floor((items - 1) / t)))), the rank estimate's weight, and
//      with every right-hand side taken before the update, for c < C-1:
//        X[u,c] += lr (L (Y[i,c] - Y[j,c]) - reg X[u,c])
//        Y[i,c] += lr (L X[u,c] - reg Y[i,c])
//        Y[j,c] += lr (-L X[u,c] - reg Y[j,c])
//      and for the bias column  Y[i,C-1] += lr (L - reg Y[i,C-1]),  Y[j,C-1] += lr (-L - reg Y[j,C-1]).  i == j cannot
//      happen (j is never a liked item of u).  The sample ends;
//   5. no violation in max_sampled trials: nothing is written, the sample counts as SATISFIED.
// The call returns (satisfied, trials): the satisfied samples and the draws consumed over all samples.  Concurrent samples
// update shared rows without atomics (Hogwild, as BPR): the positives and every sample's candidate sequence are pure functions
// of (seed, s, nnz, items), but how many candidates a sample examines depends on the factors it meets, so neither the counts
// nor the factors of a multi-sample call are reproducible.  A single-sample call and a conflict-free call are exact.
//
// Layout (sgd_group.h, shared with bpr.hip and lmf.hip): one GROUP of G = 16 / 32 / 64 lanes per sample, lane l owns columns
// l, l + G, ... (CPL per lane).  The lane's columns of the user row and of the positive row stay in registers for the whole
// sample; every dot product is a register butterfly inside the group (group_dot); no LDS on the sample path.
// A trial is draw -> liked search -> row load -> dot, each step bound by latency: the candidate's row depends on j alone, so
// its load is issued before the search (sgd_group.h group_row_contains) resolves, and a Philox block holds four candidates, so
// the draw of trial t + 1 is a register select that needs nothing from trial t (loading the NEXT candidate's row a trial
// ahead as well measured 7 - 9 % slower at C = 101 and 129 and is not done: DESIGN 4.15).  The groups of a wavefront need different
// numbers of trials, so the kernel is ONE loop whose body is one trial step of the group's current sample: a group whose
// sample ended (by update or satisfied) starts its next one, s += groups in flight, in the following pass of the same loop,
// where the other groups run their next trial.  Every pass consumes a trial, a sample has at most max_sampled of them and
// s only grows: the loop is bounded by samples x max_sampled, it never waits and shares no flag with another workgroup.
//
// Every id the kernel turns into an address has been checked on the device first (check_pair_ids, pair_sgd.hip): an id
// outside its matrix returns IMP_OUT_OF_RANGE with nothing launched.  j < items by construction.
#include "common.h"
#include "philox.h"
#include "sgd_group.h"

namespace imp {

// A store of the update: agent scope (global_store ... sc1), which writes through the XCD's L2 and does not keep the line
// there.  A plain store stays dirty in the writing XCD's L2 until the kernel ends and stays valid there afterwards; where
// workgroups on two XCDs wrote or read the same line during the call, a LATER kernel scheduled on one of them then read
// that XCD's version while memory -- and every copy to the host -- held the other's: measured, about 900 of 16 000 item
// rows after an epoch, until other traffic evicted the lines.  With these stores no row differed.
__device__ __forceinline__ void store_through(float *p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct WarpArgs {
  const int32_t *__restrict__ userids;
  const int32_t *__restrict__ itemids;
  const int32_t *__restrict__ indptr;
  float *X, *Y;  // rows are shared between concurrent samples (Hogwild): no __restrict__
  int64_t nnz, samples;
  uint64_t seed;
  float lr, reg;
  int C, items, max_sampled;
  unsigned long long *stats;  // [0] satisfied, [1] trials
};

template <int G, int CPL>
__global__ __launch_bounds__(256) void warp_update_kernel(WarpArgs a) {
  const LaneGroup<G> g;
  const int gl = g.gl;
  const int C = a.C;
  const float lr = a.lr, reg = a.reg;
  const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
  unsigned long long satisfied = 0, trials = 0;

  int64_t s = g.index;
  // the group's current sample: t trials consumed so far (0: not started), its rows, score and row of the pattern
  int t = 0;
  float *xr = nullptr, *yi = nullptr;
  float x[CPL], p[CPL];
  float sp = 0.f;
  int64_t lo = 0, hi = 0;
  u32x4 cand = {0, 0, 0, 0};  // the Philox block with the candidates of trials 4 (t >> 2) + 1 .. + 4
  while (s < a.samples) {
    const uint32_t s_lo = (uint32_t)s, s_hi = (uint32_t)((uint64_t)s >> 32);
    if (t == 0) {  // steps 1 and 2
      const u32x4 r = philox4x32_10(s_lo, s_hi, 0u, 4u, k0, k1);
      const int64_t lp = (int64_t)(((uint64_t)r.x * (uint64_t)a.nnz) >> 32);
      const int u = a.userids[lp], i = a.itemids[lp];
      cand = philox4x32_10(s_lo, s_hi, 1u, 4u, k0, k1);
      lo = a.indptr[u], hi = a.indptr[u + 1];
      xr = a.X + (size_t)u * C, yi = a.Y + (size_t)i * C;
#pragma unroll
      for (int k = 0; k < CPL; ++k) {  // the two rows column by column: not two group_loads, which would reorder the loads
        const int c = gl + G * k;
        x[k] = c < C ? xr[c] : 0.f;
        p[k] = c < C ? yi[c] : 0.f;
      }
      float part = 0.f;
#pragma unroll
      for (int k = 0; k < CPL; ++k) part = fmaf(x[k], p[k], part);
      sp = group_allsum<G>(part);  // bitwise the same in every lane of the group
    }

    // step 3, trial t + 1
    const int w = t & 3;
    const uint32_t word = w == 0 ? cand.x : w == 1 ? cand.y : w == 2 ? cand.z : cand.w;
    const int j = (int)(((uint64_t)word * (uint64_t)(uint32_t)a.items) >> 32);
    ++t;
    float *yj = a.Y + (size_t)j * C;
    float q[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) {  // in flight while the search below runs (group_load here moves 21 kernels' registers)
      const int c = gl + G * k;
      q[k] = c < C ? yj[c] : 0.f;
    }
    if (w == 3 && t < a.max_sampled) cand = philox4x32_10(s_lo, s_hi, 1u + (uint32_t)(t >> 2), 4u, k0, k1);
    bool updated = false;
    if (!group_row_contains<G>(a.itemids, lo, hi, j, gl, g.gmask)) {
      const float sn = group_dot<G>(x, q);
      if (sn > sp - 1.f) {  // step 4
        const int rank = (a.items - 1) / t;
        const float L = fminf(10.f, logf((float)(rank > 1 ? rank : 1)));
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
          const int c = gl + G * k;
          if (c < C) {
            const bool bias = c == C - 1;
            if (!bias) store_through(xr + c, x[k] + lr * (L * (p[k] - q[k]) - reg * x[k]));
            store_through(yi + c, p[k] + lr * ((bias ? L : L * x[k]) - reg * p[k]));
            store_through(yj + c, q[k] + lr * ((bias ? -L : -L * x[k]) - reg * q[k]));
          }
        }
        updated = true;
      }
    }
    if (updated || t == a.max_sampled) {  // the sample ends; without an update it is satisfied (step 5)
      satisfied += !updated && gl == 0;
      trials += gl == 0 ? t : 0;
      s += g.ngroups;
      t = 0;
    }
  }

  block_add_counts(satisfied, trials, a.stats);
}

}  // namespace imp

using namespace imp;

extern "C" int imp_warp_update(const imp_intvector *userids, const imp_intvector *itemids, const imp_intvector *indptr, imp_matrix *X,
                               imp_matrix *Y, float learning_rate, float regularization, int64_t seed, int max_sampled,
                               int64_t samples, int64_t *satisfied, int64_t *trials) {
  return guarded([&] {
    if (max_sampled < 1 || max_sampled > 4096) throw std::invalid_argument("warp_update: max_sampled must lie in 1 .. 4096");
    if (Y && Y->rows > (size_t)INT32_MAX) throw std::invalid_argument("warp_update: more than 2^31 - 1 items");
    pair_update("warp_update", "warp_check_ids", "warp_update", userids, itemids, indptr, X, Y, samples, satisfied, trials,
                [&](int G, int grid, int64_t n, unsigned long long *stats) {
                  const WarpArgs a{userids->v.data(), itemids->v.data(), indptr->v.data(), X->mut<float>(), Y->mut<float>(), (int64_t)userids->size, n,
                                   (uint64_t)seed, learning_rate, regularization, (int)X->cols, (int)Y->rows, max_sampled, stats};
                  for_group_shape<false>(G, a.C, [&](auto g, auto cpl) {
                    warp_update_kernel<decltype(g)::value, decltype(cpl)::value><<<grid, 256, 0, stream()>>>(a);
                  });
                });
  });
}
