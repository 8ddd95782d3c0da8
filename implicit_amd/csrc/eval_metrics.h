// Ranking metrics of ONE recommendation row (P@K, MAP@K, NDCG@K, AUC@K), written once for host and device.
//
// A restatement, from the equations, of the per-user body of the reference's ranking_metrics_at_k
// (implicit/evaluation.pyx:444-464).  With `likes` the user's held-out items, ids[0 .. K) the recommended row,
// pos = |likes|, neg = items - pos, h(i) the hits among positions 0 .. i and m the misses among all K:
//
//   hits   = h(K-1)
//   pr_div = min(K, pos)
//   ap     = (sum over hit positions i of h(i) / (i + 1)) / min(K, pos)
//   ndcg   = sum over hit positions i of cg[i] / cg_sum[min(K, pos) - 1]             cg[i] = 1 / log2(i + 2)
//   auc    = (sum over miss positions i of h(i)  +  (hits + pos) / 2 * (neg - m)) / (pos * neg)
//
// cg and its running sum cg_sum are tables of length K the caller supplies (numpy computes them: no log2 here).  An id that is
// negative (the -1 padding of ItemItemRecommender.recommend) or >= items is a miss.  Membership is a binary search in the
// row's sorted, unique int32 ids.  Everything is accumulated in double in position order 0 .. K-1; the miss sum of the AUC
// is a sum of integers below 2^53 and therefore exact in any order.
//
// The row is consumed in chunks of up to 64 positions described by a hit mask (bit j: position base + j is a hit).  The host
// fills the mask position by position; the kernel (evaluation.hip) gets it from one ballot over lanes that each test one
// position.  Both then run the same EvalRowAcc code, so the two paths perform the same double operations in the same order.
#ifndef IMPLICIT_AMD_CSRC_EVAL_METRICS_H_
#define IMPLICIT_AMD_CSRC_EVAL_METRICS_H_

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IMP_EVAL_HD __host__ __device__ inline
#else
#define IMP_EVAL_HD inline
#endif

namespace imp {

struct EvalRow {
  double hits;    // relevant recommendations of the row
  double pr_div;  // min(K, pos)
  double ap;      // the row's term of sum_ap
  double ndcg;    // ... of sum_ndcg
  double auc;     // ... of sum_auc
};

// is `id` one of likes[0 .. n) (strictly increasing)?
IMP_EVAL_HD bool eval_is_liked(int32_t id, const int32_t *likes, int64_t n, int32_t items) {
  if (id < 0 || id >= items) return false;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (likes[mid] < id) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && likes[lo] == id;
}

struct EvalRowAcc {
  double hit = 0, miss = 0, miss_hits = 0, ap = 0, ndcg = 0, idcg = 1;

  // pos >= 1 (a row without held-out items is never evaluated)
  IMP_EVAL_HD void begin(int K, int64_t pos, const double *cg_sum) {
    hit = miss = miss_hits = ap = ndcg = 0;
    idcg = cg_sum[(pos < K ? (int)pos : K) - 1];
  }

  // positions base .. base + count - 1 (count <= 64), bit j of `mask` set when position base + j is a hit
  IMP_EVAL_HD void chunk(uint64_t mask, int base, int count, const double *cg) {
    int at = 0;  // first position of the chunk not yet accounted for
    while (mask) {
      const int j = __builtin_ctzll(mask);
      const double gap = (double)(j - at);  // misses since the previous hit: each adds the hits so far
      miss += gap;
      miss_hits += hit * gap;
      hit += 1;
      ap += hit / (double)(base + j + 1);
      ndcg += cg[base + j] / idcg;
      mask &= ~((uint64_t)1 << j);
      at = j + 1;
    }
    const double gap = (double)(count - at);
    miss += gap;
    miss_hits += hit * gap;
  }

  IMP_EVAL_HD EvalRow finish(int K, int64_t pos, int32_t items) const {
    const double p = (double)pos, n = (double)items - p, div = (double)(pos < K ? pos : (int64_t)K);
    EvalRow r;
    r.hits = hit;
    r.pr_div = div;
    r.ap = ap / div;
    r.ndcg = ndcg;
    r.auc = (miss_hits + ((hit + p) / 2.0) * (n - miss)) / (p * n);
    return r;
  }
};

// The whole row in one call: ids[0 .. K) against likes[0 .. pos), pos >= 1.
IMP_EVAL_HD EvalRow eval_row(const int32_t *ids, int K, const int32_t *likes, int64_t pos, int32_t items, const double *cg,
                             const double *cg_sum) {
  EvalRowAcc acc;
  acc.begin(K, pos, cg_sum);
  for (int base = 0; base < K; base += 64) {
    const int count = K - base < 64 ? K - base : 64;
    uint64_t mask = 0;
    for (int j = 0; j < count; ++j)
      if (eval_is_liked(ids[base + j], likes, pos, items)) mask |= (uint64_t)1 << j;
    acc.chunk(mask, base, count, cg);
  }
  return acc.finish(K, pos, items);
}

}  // namespace imp

#endif  // IMPLICIT_AMD_CSRC_EVAL_METRICS_H_
