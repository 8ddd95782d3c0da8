// Ranking metrics (P@K, MAP@K, NDCG@K, AUC@K) of recommendation rows that are already on the device.
//
// The reference evaluates on the host: per batch of 1000 users it downloads the ids model.recommend produced and walks them
// against a hash set of the user's held-out items (implicit/evaluation.pyx:423-466).  Here the ids stay where
// KnnQuery.topk_device left them; imp_eval_add queues one kernel over them and a second that folds its partial sums into six
// running doubles held by the handle, and nothing is read back before imp_eval_result.  The per-row arithmetic is
// eval_metrics.h, shared with imp_host_ranking_metrics below (plain host code: it pins the numbers where there is no GPU).
//
// Kernel mapping.  Lanes are rank positions: a group of G = min(64, next power of two >= k) lanes serves one row, so a
// wavefront handles 64 / G rows and a workgroup of 256 threads a tile of 256 / G.  Each lane tests its id against the user's
// sorted held-out ids (binary search), one ballot gives the wavefront's hit mask and the group's leader runs the shared
// accumulator over its G bits; for k > 64 the group walks the row in chunks of 64 and the accumulator carries the counts.
// No floating-point atomics anywhere: the leaders put their rows' terms into LDS, six threads add them up in row order,
// every workgroup strides over the tiles with its sums in registers and writes ONE workspace slot; the single workgroup of
// the fold kernel adds the slots in a fixed order.  The same call on the same data therefore gives the same bits every time.
#include <algorithm>
#include <cstring>

#include "common.h"
#include "eval_metrics.h"

struct imp_eval {
  int32_t rows = 0, cols = 0;
  int k = 0;
  imp::DeviceArray<int64_t> indptr;  // rows + 1 offsets into `indices`
  imp::DeviceArray<int32_t> indices;
  imp::DeviceArray<double> tables;   // cg[k], then cg_sum[k]
  imp::DeviceArray<double> sums;     // relevant, pr_div, sum_ap, sum_ndcg, sum_auc, total
  imp::DeviceArray<double> slots;    // [kEvalMaxGrid][6] partial sums of one add
};

namespace imp {

constexpr int kEvalBlock = 256;
constexpr int kEvalMaxGrid = 1024;
constexpr int kEvalSums = 6;

// The held-out pattern as both entry points take it: offsets of either width (rebased to 0), every row strictly increasing
// inside [0, cols).  Returns the 64-bit offsets.
static std::vector<int64_t> eval_check_pattern(const char *who, int32_t rows, int32_t cols, const void *indptr, int indptr_is_64,
                                               const int32_t *indices, int k, const double *cg, const double *cg_sum) {
  const std::string w(who);
  if (rows < 0 || cols < 0) throw std::invalid_argument(w + ": negative dimension");
  if (k < 1) throw std::invalid_argument(w + ": k must be >= 1");
  if (!indptr || !cg || !cg_sum) throw std::invalid_argument(w + ": NULL array");
  const int64_t *p64 = indptr_is_64 ? static_cast<const int64_t *>(indptr) : nullptr;
  const int32_t *p32 = indptr_is_64 ? nullptr : static_cast<const int32_t *>(indptr);
  std::vector<int64_t> off((size_t)rows + 1);
  for (int64_t r = 0; r <= rows; ++r) off[r] = p64 ? p64[r] : (int64_t)p32[r];
  if (off[0] != 0) throw std::invalid_argument(w + ": indptr must start at 0");
  if (off[rows] && !indices) throw std::invalid_argument(w + ": NULL array");
  for (int32_t r = 0; r < rows; ++r) {
    if (off[r + 1] < off[r]) throw std::invalid_argument(w + ": indptr must be non-decreasing");
    int64_t prev = -1;
    for (int64_t p = off[r]; p < off[r + 1]; ++p) {
      const int64_t c = indices[p];
      if (c < 0 || c >= cols) throw std::invalid_argument(w + ": column id out of range");
      if (c <= prev) throw std::invalid_argument(w + ": the column ids of a row must be strictly increasing");
      prev = c;
    }
  }
  return off;
}

struct EvalArgs {
  const int64_t *indptr;
  const int32_t *indices;
  const double *cg, *cg_sum;
  const int32_t *ids;      // [n][k]
  const int32_t *userids;  // [n]
  double *per_row;         // [n][4] or nullptr
  double *slots;           // [gridDim.x][6]
  int64_t n;
  int32_t rows, cols;
  int k;
};

// G lanes per row (a power of two <= 64, >= k unless G = 64)
template <int G> __global__ __launch_bounds__(kEvalBlock) void eval_rows_kernel(const EvalArgs a) {
  constexpr int kTile = kEvalBlock / G;  // rows per workgroup and step
  __shared__ double terms[kTile][kEvalSums];
  const int lane = threadIdx.x & 63, sub = threadIdx.x & (G - 1), slot = threadIdx.x / G;
  const int shift = lane & ~(G - 1);  // first lane of this group within the wavefront
  const int64_t tiles = (a.n + kTile - 1) / kTile;
  double run = 0;  // threads 0 .. 5: this workgroup's sum of quantity threadIdx.x
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r = tile * kTile + slot;
    // a row that is past the end, names no row of the pattern or has nothing held out is never looked up
    int64_t begin = 0, pos = 0;
    if (r < a.n) {
      const int32_t u = a.userids[r];
      if (u >= 0 && u < a.rows) begin = a.indptr[u], pos = a.indptr[u + 1] - begin;
    }
    const bool live = pos > 0;
    EvalRowAcc acc;
    if (live && sub == 0) acc.begin(a.k, pos, a.cg_sum);
    for (int base = 0; base < a.k; base += 64) {  // the trip count depends on k alone: every lane reaches the ballot
      const int p = base + sub;
      bool hit = false;
      if (live && p < a.k) hit = eval_is_liked(a.ids[r * a.k + p], a.indices + begin, pos, a.cols);
      const uint64_t wave = __ballot(hit);
      if (live && sub == 0) {
        const uint64_t mask = G == 64 ? wave : (wave >> shift) & (((uint64_t)1 << (G & 63)) - 1);
        acc.chunk(mask, base, min(64, a.k - base), a.cg);
      }
    }
    if (sub == 0) {
      EvalRow row = {0, 0, 0, 0, 0};
      if (live) row = acc.finish(a.k, pos, a.cols);
      terms[slot][0] = row.hits, terms[slot][1] = row.pr_div, terms[slot][2] = row.ap, terms[slot][3] = row.ndcg;
      terms[slot][4] = row.auc, terms[slot][5] = live ? 1.0 : 0.0;
      if (a.per_row && r < a.n) {
        double *o = a.per_row + r * 4;
        o[0] = row.hits, o[1] = row.ap, o[2] = row.ndcg, o[3] = row.auc;
      }
    }
    __syncthreads();
    if (threadIdx.x < kEvalSums)
      for (int s = 0; s < kTile; ++s) run += terms[s][threadIdx.x];  // row order; rows that do not count hold zeros
    __syncthreads();
  }
  if (threadIdx.x < kEvalSums) a.slots[(size_t)blockIdx.x * kEvalSums + threadIdx.x] = run;
}

// One workgroup: thread t adds slots t, t + 256, ... in that order, a fixed tree adds the 256 partial sums, thread 0 adds the
// result to the running sum.
__global__ __launch_bounds__(kEvalBlock) void eval_fold_kernel(const double *__restrict__ slots, int n_slots, double *__restrict__ sums) {
  __shared__ double part[kEvalSums][kEvalBlock];
  double s[kEvalSums] = {0, 0, 0, 0, 0, 0};
  for (int j = threadIdx.x; j < n_slots; j += kEvalBlock)
    for (int q = 0; q < kEvalSums; ++q) s[q] += slots[(size_t)j * kEvalSums + q];
  for (int q = 0; q < kEvalSums; ++q) part[q][threadIdx.x] = s[q];
  __syncthreads();
  for (int w = kEvalBlock / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
      for (int q = 0; q < kEvalSums; ++q) part[q][threadIdx.x] += part[q][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x < kEvalSums) sums[threadIdx.x] += part[threadIdx.x][0];
}

template <int G> static void launch_eval_rows(const EvalArgs &a, int grid) {
  hipLaunchKernelGGL(eval_rows_kernel<G>, dim3(grid), dim3(kEvalBlock), 0, stream(), a);
}

}  // namespace imp

using namespace imp;

extern "C" int imp_eval_create(int32_t rows, int32_t cols, const void *indptr, int indptr_is_64, const int32_t *indices, int k,
                               const double *cg, const double *cg_sum, imp_eval **out) {
  return guarded([&] {
    if (!out) throw std::invalid_argument("eval_create: NULL output handle");
    const std::vector<int64_t> off = eval_check_pattern("eval_create", rows, cols, indptr, indptr_is_64, indices, k, cg, cg_sum);
    auto e = std::make_unique<imp_eval>();
    e->rows = rows, e->cols = cols, e->k = k;
    std::vector<double> tables((size_t)2 * k);
    std::copy(cg, cg + k, tables.begin());
    std::copy(cg_sum, cg_sum + k, tables.begin() + k);
    e->indptr.upload(off.data(), off.size());
    e->indices.upload(indices, (size_t)off[rows]);
    e->tables.upload(tables.data(), tables.size());
    e->sums.alloc(kEvalSums, true);
    e->slots.alloc((size_t)kEvalMaxGrid * kEvalSums);
    sync();  // the uploads read this call's host vectors
    *out = e.release();
  });
}

extern "C" int imp_eval_add(imp_eval *e, const imp_matrix *ids, const imp_intvector *userids, double *per_row) {
  return guarded([&] {
    if (!e || !ids || !userids) throw std::invalid_argument("eval_add: NULL argument");
    if (ids->itemsize != 4) throw std::invalid_argument("eval_add: ids must be a matrix of 4-byte elements (int32 bit patterns)");
    if (ids->cols != (size_t)e->k) throw std::invalid_argument("eval_add: ids must have k columns");
    if (ids->rows != userids->size) throw std::invalid_argument("eval_add: one user id per row of ids");
    const int64_t n = (int64_t)ids->rows;
    if (n == 0) return;
    DeviceArray<double> rows_out;
    if (per_row) rows_out.alloc((size_t)n * 4);
    int G = 1;
    while (G < e->k && G < 64) G <<= 1;
    const int64_t tiles = (n + kEvalBlock / G - 1) / (kEvalBlock / G);
    const int grid = (int)std::min<int64_t>(tiles, kEvalMaxGrid);
    const EvalArgs a{e->indptr.data(), e->indices.data(), e->tables.data(), e->tables.data() + e->k,
                     ids->as<int32_t>(), userids->v.data(), rows_out.data(), e->slots.data(), n,
                     e->rows, e->cols, e->k};
    {
      IMP_PROF("eval_rows");
      switch (G) {
        case 1: launch_eval_rows<1>(a, grid); break;
        case 2: launch_eval_rows<2>(a, grid); break;
        case 4: launch_eval_rows<4>(a, grid); break;
        case 8: launch_eval_rows<8>(a, grid); break;
        case 16: launch_eval_rows<16>(a, grid); break;
        case 32: launch_eval_rows<32>(a, grid); break;
        default: launch_eval_rows<64>(a, grid); break;
      }
      IMP_CHECK_HIP(hipGetLastError());
    }
    {
      IMP_PROF("eval_fold");
      hipLaunchKernelGGL(eval_fold_kernel, dim3(1), dim3(kEvalBlock), 0, stream(), e->slots.data(), grid, e->sums.data());
      IMP_CHECK_HIP(hipGetLastError());
    }
    if (per_row) {  // the only case with a host wait: the caller reads the rows now
      IMP_CHECK_HIP(hipMemcpyAsync(per_row, rows_out.data(), (size_t)n * 4 * sizeof(double), hipMemcpyDeviceToHost, stream()));
      sync();
    }
  });
}

extern "C" int imp_eval_result(imp_eval *e, double *out) {
  return guarded([&] {
    if (!e || !out) throw std::invalid_argument("eval_result: NULL argument");
    IMP_CHECK_HIP(hipMemcpyAsync(out, e->sums.data(), kEvalSums * sizeof(double), hipMemcpyDeviceToHost, stream()));
    sync();
  });
}

extern "C" int imp_eval_reset(imp_eval *e) {
  return guarded([&] {
    if (!e) throw std::invalid_argument("eval_reset: NULL argument");
    IMP_CHECK_HIP(hipMemsetAsync(e->sums.data(), 0, kEvalSums * sizeof(double), stream()));
  });
}

extern "C" int imp_eval_destroy(imp_eval *e) {
  return guarded([&] { delete e; });
}

// The same sums for n rows on the host, in row order, through the same per-row function.
extern "C" int imp_host_ranking_metrics(int32_t rows, int32_t cols, const void *indptr, int indptr_is_64, const int32_t *indices,
                                        int k, const double *cg, const double *cg_sum, const int32_t *ids, const int32_t *userids,
                                        int64_t n, double *sums, double *per_row) {
  return guarded_host([&] {
    const std::vector<int64_t> off =
        eval_check_pattern("host_ranking_metrics", rows, cols, indptr, indptr_is_64, indices, k, cg, cg_sum);
    if (n < 0) throw std::invalid_argument("host_ranking_metrics: negative row count");
    if (!sums || (n && (!ids || !userids))) throw std::invalid_argument("host_ranking_metrics: NULL array");
    for (int64_t r = 0; r < n; ++r)
      if (userids[r] < 0 || userids[r] >= rows) throw out_of_range_error("host_ranking_metrics: user id outside the test matrix");
    double s[kEvalSums] = {0, 0, 0, 0, 0, 0};
    for (int64_t r = 0; r < n; ++r) {
      const int64_t begin = off[userids[r]], pos = off[userids[r] + 1] - begin;
      EvalRow row = {0, 0, 0, 0, 0};
      if (pos > 0) {
        row = eval_row(ids + r * k, k, indices + begin, pos, cols, cg, cg_sum);
        s[0] += row.hits, s[1] += row.pr_div, s[2] += row.ap, s[3] += row.ndcg, s[4] += row.auc, s[5] += 1.0;
      }
      if (per_row) per_row[r * 4 + 0] = row.hits, per_row[r * 4 + 1] = row.ap, per_row[r * 4 + 2] = row.ndcg, per_row[r * 4 + 3] = row.auc;
    }
    std::copy(s, s + kEvalSums, sums);
  });
}
