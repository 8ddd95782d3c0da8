// K21: WARP-loss factorization over user and item features -- one SGD epoch in which a user and an item are the weighted
// sums of the embeddings of their features (imp_hybrid_warp_update).
//
// No reference counterpart: the model is Kula, "Metadata Embeddings for User and Item Cold-start Recommendations" (CBRecSys
// 2015) under the loss of warp.hip.  userids / itemids / indptr are the interaction pattern exactly as imp_warp_update takes
// it (COO ids, row pointers, row indices sorted, nnz < 2^31).  user_features (users x UF) and item_features (items x IF) are
// CSR matrices with fp32 values and no repeated column within a row; EU (UF x C) and EI (IF x C) are float32 embeddings with
// C = factors + 1, 2 <= C <= 1024.
//   Representations.  For user u and c < C-1:  x[c] = sum over row u of user_features, in stored order, of w_a EU[a,c] -- the
//   fp32 chain acc = fmaf(w_a, EU[a,c], acc) from 0.  x[C-1] = 1.0 by definition: column C-1 of EU is never read or written.
//   For item i and every c < C:  y_i[c] is the same chain over row i of item_features and EI; column C-1 is the item bias, the
//   weighted sum of the feature biases.  An empty feature row is legal and gives the zero vector (x[C-1] stays 1.0).
// Sample s of a call, 0 <= s < samples:
//   1. the positive of warp.hip step 1 with 5 as the fourth Philox counter word (philox.h): r = Philox(counter (s_lo, s_hi, 0,
//      5), key (seed_lo, seed_hi));  lp = (r.x * nnz) >> 32;  u = userids[lp], i = itemids[lp];
//   2. sp = sum_{c < C} x[c] y_i[c];
//   3. trials t = 1 .. max_sampled (1 <= max_sampled <= 4096): word (t-1) & 3 of Philox(counter (s_lo, s_hi, 1 + ((t-1) >> 2),
//      5), same key) gives j = (word * items) >> 32.  j in row u of the pattern: the trial is consumed, nothing else happens.
//      Otherwise sn = sum_c x[c] y_j[c] and the trial VIOLATES when sn > sp - 1;
//   4. on the first violating trial t:  L = min(10, log(max(1, floor((items - 1) / t)))), and with every right-hand side
//      taken before the update the gradients of the three representations are, for c < C-1,
//        g_x[c] = L (y_i[c] - y_j[c]),  g_i[c] = L x[c],  g_j[c] = -L x[c],   and in the bias column  g_i = L,  g_j = -L.
//      Every stored feature (a, w) of a row then takes  E[a,c] += lr (w g[c] - reg E[a,c]):  row u of user_features into EU
//      (c < C-1) with g_x, row i of item_features into EI with g_i, row j with g_j.  THE NEGATIVE'S SCATTER RUNS AFTER THE
//      POSITIVE'S AND RE-READS THE ROWS IT UPDATES: a feature that i and j share receives both steps, in that order, the
//      second on the value the first left.  The sample ends;
//   5. no violation in max_sampled trials: nothing is written, the sample counts as SATISFIED.
// The call returns (satisfied, trials) as imp_warp_update does.  With one feature of weight 1 per row (identity feature
// matrices) the update is algebraically imp_warp_update's.  Concurrent samples update shared embedding rows without atomics
// (Hogwild): a single-sample call and a conflict-free call are exact, a multi-sample call is not reproducible.
//
// Design.  The lane-group layout of sgd_group.h: G = 16 / 32 / 64 lanes per sample, lane l owns columns l,
// l + G, ... in CPL registers, so every embedding row is read and written coalesced and every dot product is a register
// butterfly.  x and y_i are accumulated once per sample and stay in registers, as does the candidate's y_j from its gather to
// its scatter.
//   A feature row is held by the group as a GroupRow: its range and, in lane l, the id and weight of its entry l -- one
//   coalesced load of ids and one of weights per G entries.  The walk (for_feature_batches) broadcasts them to the group by
//   __shfl, kFlight entries at a time, and the body issues the kFlight x CPL loads of those embedding rows together before it
//   uses the first: kFlight = 4 rows up to CPL = 4 and 2 above, 4 .. 32 loads in flight per lane.  Rows of more than G
//   features go round the outer loop, which loads the next G ids and weights.
//   The three GroupRows of a sample (u, i and the candidate j) are kept from the gather to the scatter: up to G features per
//   row the scatter loads no id and no weight.  The embedding rows themselves are NOT kept: the contract's order makes the
//   negative's scatter read what the positive's left in a shared feature, telling a shared feature from another costs an
//   nf_i x nf_j comparison, and the lines were gathered a few hundred cycles earlier, so the scatter re-reads every row it
//   updates (kFlight rows in flight again: the rows of one feature row are distinct, so loading a batch before storing it is
//   safe).  Longer rows take the same path with their ids re-read.
//   A trial is draw -> ids of the candidate's features -> liked search -> gather -> dot.  The candidate's GroupRow depends on j
//   alone and is issued before the search (group_row_contains) resolves; the embedding rows it names cannot be issued before
//   those ids arrive, and a liked candidate skips the gather.  The kernel is warp.hip's single divergent loop, one trial step
//   per pass, a group starting its next sample independently; it is bounded by samples x max_sampled, never waits and shares
//   no flag with another workgroup.  The gathers and scatters are loops with group-uniform trip counts inside that body.
//   Samples in flight: hogwild_in_flight over (UF, IF) -- the contended rows are feature embeddings.
//
// Every id the kernel turns into an address has been checked on the device first: the interaction ids by check_pair_ids
// (pair_sgd.hip), the feature column ids by feature_check_kernel; an id outside its matrix returns IMP_OUT_OF_RANGE with
// nothing launched.  j < items by construction.
#include "common.h"
#include "philox.h"
#include "sgd_group.h"

namespace imp {

struct FeatureRows {  // a feature matrix on the device
  const int32_t *__restrict__ indptr;
  const int32_t *__restrict__ ids;
  const float *__restrict__ w;
};

// One feature row as its group holds it: entries [b, e) of the matrix, and in lane l the id and weight of entry b + l (0 past
// the row's end).
struct GroupRow {
  int b, e, id;
  float w;
};

__device__ __forceinline__ GroupRow open_row(const FeatureRows &f, int row, int gl) {
  GroupRow r;
  r.b = f.indptr[row], r.e = f.indptr[row + 1];
  const bool in = r.b + gl < r.e;
  r.id = in ? f.ids[r.b + gl] : 0;
  r.w = in ? f.w[r.b + gl] : 0.f;
  return r;
}

// body(a, w, n) for the row's entries in stored order, F at a time: ids a[0 .. n) with weights w[0 .. n), 1 <= n <= F (a[n ..
// F) are ids of the matrix too, so their addresses are valid, but they are not part of the row).  Every lane of the group
// calls it with the same row; trip counts are group-uniform, so the lanes a __shfl reads are active.
template <int G, int F, typename Body>
__device__ __forceinline__ void for_feature_batches(const FeatureRows &f, const GroupRow &r, int gl, Body body) {
  for (int base = r.b; base < r.e; base += G) {
    int id = r.id;
    float w = r.w;
    if (base != r.b) {  // beyond the G entries the GroupRow holds
      const bool in = base + gl < r.e;
      id = in ? f.ids[base + gl] : 0;
      w = in ? f.w[base + gl] : 0.f;
    }
    const int n = r.e - base < G ? r.e - base : G;
    for (int k = 0; k < n; k += F) {
      int a[F];
      float wk[F];
#pragma unroll
      for (int j = 0; j < F; ++j) {
        a[j] = __shfl(id, (k + j) & (G - 1), G);
        wk[j] = __shfl(w, (k + j) & (G - 1), G);
      }
      body(a, wk, n - k < F ? n - k : F);
    }
  }
}

// the lane's columns (below Cw) of the embedding rows a[0 .. n), all loads issued together
template <int G, int CPL, int F>
__device__ __forceinline__ void load_batch(const float *E, int C, int Cw, int gl, const int (&a)[F], int n, float (&e)[F][CPL]) {
#pragma unroll
  for (int j = 0; j < F; ++j)
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int c = gl + G * k;
      e[j][k] = j < n && c < Cw ? E[(size_t)a[j] * C + c] : 0.f;
    }
}

// acc = the representation of the row: columns below Cw of sum w_a E[a, .], the fmaf chain in stored order from 0
template <int G, int CPL, int F>
__device__ __forceinline__ void group_represent(const FeatureRows &f, const GroupRow &r, const float *E, int C, int Cw, int gl,
                                                float (&acc)[CPL]) {
#pragma unroll
  for (int k = 0; k < CPL; ++k) acc[k] = 0.f;
  for_feature_batches<G, F>(f, r, gl, [&](const int(&a)[F], const float(&w)[F], int n) {
    float e[F][CPL];
    load_batch<G, CPL, F>(E, C, Cw, gl, a, n, e);
#pragma unroll
    for (int j = 0; j < F; ++j)
      if (j < n) {
#pragma unroll
        for (int k = 0; k < CPL; ++k) acc[k] = fmaf(w[j], e[j][k], acc[k]);
      }
  });
}

// E[a, c] += lr (w g[c] - reg E[a, c]) for every stored (a, w) of the row and c < Cw, each row read again here
template <int G, int CPL, int F>
__device__ __forceinline__ void group_scatter(const FeatureRows &f, const GroupRow &r, float *E, int C, int Cw, int gl,
                                              const float (&g)[CPL], float lr, float reg) {
  for_feature_batches<G, F>(f, r, gl, [&](const int(&a)[F], const float(&w)[F], int n) {
    float e[F][CPL];
    load_batch<G, CPL, F>(E, C, Cw, gl, a, n, e);
#pragma unroll
    for (int j = 0; j < F; ++j)
      if (j < n) {
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
          const int c = gl + G * k;
          if (c < Cw) store_through(E + (size_t)a[j] * C + c, e[j][k] + lr * (w[j] * g[k] - reg * e[j][k]));
        }
      }
  });
}

struct HybridArgs {
  const int32_t *__restrict__ userids;
  const int32_t *__restrict__ itemids;
  const int32_t *__restrict__ indptr;
  FeatureRows uf, itf;
  float *EU, *EI;  // rows are shared between concurrent samples (Hogwild): no __restrict__
  int64_t nnz, samples;
  uint64_t seed;
  float lr, reg;
  int C, items, max_sampled;
  unsigned long long *stats;  // [0] satisfied, [1] trials
};

constexpr uint32_t kHybridTag = 5;  // philox.h

template <int G, int CPL>
__global__ __launch_bounds__(256) void hybrid_warp_kernel(HybridArgs a) {
  constexpr int kFlight = CPL <= 4 ? 4 : 2;  // embedding rows in flight per lane
  const LaneGroup<G> g;
  const int gl = g.gl;
  const int C = a.C;
  const float lr = a.lr, reg = a.reg;
  const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
  unsigned long long satisfied = 0, trials = 0;

  int64_t s = g.index;
  // the group's current sample: t trials consumed so far (0: not started), its feature rows, representations, score and row
  // of the pattern
  int t = 0;
  GroupRow ur = {0, 0, 0, 0.f}, ir = {0, 0, 0, 0.f};
  float x[CPL], p[CPL];
  float sp = 0.f;
  int64_t lo = 0, hi = 0;
  u32x4 cand = {0, 0, 0, 0};  // the Philox block with the candidates of trials 4 (t >> 2) + 1 .. + 4
  while (s < a.samples) {
    const uint32_t s_lo = (uint32_t)s, s_hi = (uint32_t)((uint64_t)s >> 32);
    if (t == 0) {  // steps 1 and 2
      const u32x4 r = philox4x32_10(s_lo, s_hi, 0u, kHybridTag, k0, k1);
      const int64_t lp = (int64_t)(((uint64_t)r.x * (uint64_t)a.nnz) >> 32);
      const int u = a.userids[lp], i = a.itemids[lp];
      cand = philox4x32_10(s_lo, s_hi, 1u, kHybridTag, k0, k1);
      lo = a.indptr[u], hi = a.indptr[u + 1];
      ur = open_row(a.uf, u, gl), ir = open_row(a.itf, i, gl);
      group_represent<G, CPL, kFlight>(a.uf, ur, a.EU, C, C - 1, gl, x);
      group_represent<G, CPL, kFlight>(a.itf, ir, a.EI, C, C, gl, p);
#pragma unroll
      for (int k = 0; k < CPL; ++k)
        if (gl + G * k == C - 1) x[k] = 1.f;
      sp = group_dot<G>(x, p);  // bitwise the same in every lane of the group
    }

    // step 3, trial t + 1
    const int w = t & 3;
    const uint32_t word = w == 0 ? cand.x : w == 1 ? cand.y : w == 2 ? cand.z : cand.w;
    const int j = (int)(((uint64_t)word * (uint64_t)(uint32_t)a.items) >> 32);
    ++t;
    const GroupRow jr = open_row(a.itf, j, gl);  // in flight while the search below runs
    if (w == 3 && t < a.max_sampled) cand = philox4x32_10(s_lo, s_hi, 1u + (uint32_t)(t >> 2), kHybridTag, k0, k1);
    bool updated = false;
    if (!group_row_contains<G>(a.itemids, lo, hi, j, gl, g.gmask)) {
      float q[CPL];
      group_represent<G, CPL, kFlight>(a.itf, jr, a.EI, C, C, gl, q);
      const float sn = group_dot<G>(x, q);
      if (sn > sp - 1.f) {  // step 4: every gradient from x, p, q as gathered, then the three scatters in the contract's order
        const int rank = (a.items - 1) / t;
        const float L = fminf(10.f, logf((float)(rank > 1 ? rank : 1)));
        float gx[CPL], gi[CPL];
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
          gx[k] = L * (p[k] - q[k]);
          gi[k] = L * x[k];  // the bias column: x is 1.0 there
        }
        group_scatter<G, CPL, kFlight>(a.uf, ur, a.EU, C, C - 1, gl, gx, lr, reg);
        group_scatter<G, CPL, kFlight>(a.itf, ir, a.EI, C, C, gl, gi, lr, reg);
#pragma unroll
        for (int k = 0; k < CPL; ++k) gi[k] = -gi[k];
        group_scatter<G, CPL, kFlight>(a.itf, jr, a.EI, C, C, gl, gi, lr, reg);
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

// The pre-pass over the feature matrices: 0 <= column id < cols.  Violations OR bits 1 (user features) / 2 (item features)
// into *bad.
__global__ __launch_bounds__(256) void feature_check_kernel(const int32_t *__restrict__ uf_ids, int64_t uf_nnz, int uf_cols,
                                                            const int32_t *__restrict__ if_ids, int64_t if_nnz, int if_cols,
                                                            unsigned long long *bad) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  unsigned flags = 0;
  for (int64_t k = tid; k < uf_nnz; k += stride)
    if (uf_ids[k] < 0 || uf_ids[k] >= uf_cols) flags |= 1;
  for (int64_t k = tid; k < if_nnz; k += stride)
    if (if_ids[k] < 0 || if_ids[k] >= if_cols) flags |= 2;
  if (flags) atomicOr(bad, (unsigned long long)flags);
}

static void check_feature_ids(const imp_csr *uf, const imp_csr *itf, unsigned long long *bad_word) {
  {
    IMP_PROF("hybrid_warp_check_features");
    const int64_t work = std::max<int64_t>(1, std::max(uf->nnz, itf->nnz));
    const int grid = (int)std::min<int64_t>((work + 255) / 256, ctx().num_cus * 8);
    feature_check_kernel<<<grid, 256, 0, stream()>>>(uf->indices.data(), uf->nnz, uf->cols, itf->indices.data(), itf->nnz, itf->cols,
                                                     bad_word);
    IMP_CHECK_HIP(hipGetLastError());
  }
  unsigned long long bad = 0;
  IMP_CHECK_HIP(hipMemcpyAsync(&bad, bad_word, sizeof(bad), hipMemcpyDeviceToHost, stream()));
  sync();
  if (bad & 1) throw out_of_range_error("hybrid_warp_update: a user feature id is outside [0, EU.rows)");
  if (bad & 2) throw out_of_range_error("hybrid_warp_update: an item feature id is outside [0, EI.rows)");
}

}  // namespace imp

using namespace imp;

extern "C" int imp_hybrid_warp_update(const imp_intvector *userids, const imp_intvector *itemids, const imp_intvector *indptr,
                                      const imp_csr *user_features, const imp_csr *item_features, imp_matrix *EU, imp_matrix *EI,
                                      float learning_rate, float regularization, int64_t seed, int max_sampled, int64_t samples,
                                      int64_t *satisfied, int64_t *trials) {
  return guarded([&] {
    const std::string w("hybrid_warp_update");
    if (!userids || !itemids || !indptr || !user_features || !item_features || !EU || !EI || !satisfied || !trials)
      throw std::invalid_argument(w + ": NULL argument");
    if (max_sampled < 1 || max_sampled > 4096) throw std::invalid_argument(w + ": max_sampled must lie in 1 .. 4096");
    if (EU->cols != EI->cols) throw std::invalid_argument(w + ": EU and EI should have the same number of columns");
    if (EU->cols < 2 || EU->cols > 1024)
      throw std::invalid_argument(w + ": embedding matrices need 2 .. 1024 columns (factors + 1 for the item bias)");
    if (EU->itemsize != 4 || EI->itemsize != 4) throw std::invalid_argument(w + ": embedding matrices must be float32");
    if (EU->overlaps(EI)) throw std::invalid_argument(w + ": EU and EI must not share storage");
    if (!user_features->parts.empty() || !item_features->parts.empty())
      throw std::invalid_argument(w + ": a feature matrix with more than 2^31 - 1 nonzeros is not supported");
    if (userids->size != itemids->size) throw std::invalid_argument("userids and itemids should have same number of elements");
    if (indptr->size != (size_t)user_features->rows + 1)
      throw std::invalid_argument(w + ": indptr must have user_features.rows + 1 entries");
    if ((size_t)user_features->cols != EU->rows) throw std::invalid_argument(w + ": EU needs one row per column of user_features");
    if ((size_t)item_features->cols != EI->rows) throw std::invalid_argument(w + ": EI needs one row per column of item_features");
    const int64_t nnz = (int64_t)userids->size;
    if (nnz > INT32_MAX) throw std::invalid_argument(w + ": more than 2^31 - 1 nonzeros");
    const int64_t n = samples < 0 ? nnz : samples;
    *satisfied = *trials = 0;
    if (nnz == 0 || n == 0) return;

    unsigned long long *stats = ctx().pair_stats.reserve(3);
    IMP_CHECK_HIP(hipMemsetAsync(stats, 0, 3 * sizeof(unsigned long long), stream()));
    check_pair_ids("hybrid_warp_update", "hybrid_warp_check_ids", userids, itemids, indptr, (size_t)user_features->rows,
                   (size_t)item_features->rows, stats + 2);
    check_feature_ids(user_features, item_features, stats + 2);

    {
      IMP_PROF("hybrid_warp_update");
      const int C = (int)EU->cols;
      const int G = pair_group_lanes(C);
      const int cap = ctx().num_cus * 8;  // 8 workgroups of 4 waves per CU: the most the CU holds
      // the contended rows are feature embeddings, not user and item rows: DESIGN 4.21
      const int64_t in_flight = hogwild_in_flight(n, EU->rows, EI->rows);
      const int grid = (int)std::min<int64_t>((in_flight * G + 255) / 256, cap);
      const HybridArgs a{userids->v.data(), itemids->v.data(), indptr->v.data(),
                         {user_features->indptr.data(), user_features->indices.data(), user_features->data.data()},
                         {item_features->indptr.data(), item_features->indices.data(), item_features->data.data()},
                         EU->mut<float>(), EI->mut<float>(), nnz, n, (uint64_t)seed, learning_rate, regularization, C,
                         (int)item_features->rows, max_sampled, stats};
      for_group_shape<false>(G, C, [&](auto g, auto cpl) {
        hybrid_warp_kernel<decltype(g)::value, decltype(cpl)::value><<<grid, 256, 0, stream()>>>(a);
      });
      IMP_CHECK_HIP(hipGetLastError());
    }
    unsigned long long h[2];
    IMP_CHECK_HIP(hipMemcpyAsync(h, stats, sizeof(h), hipMemcpyDeviceToHost, stream()));
    sync();  // synchronous in deferred mode too: the counts are the result
    *satisfied = (int64_t)h[0];
    *trials = (int64_t)h[1];
  });
}
