// K11: sparse x sparse product with a per-row top-k (imp_sparse_topk_product) -- the item-item nearest-neighbour models.
//
// Contract.  A (R x U) and B (U x C) are fp64-valued CSR matrices with int64 offsets and int32 column ids.  For every row r
// of A the TOUCHED columns are those j reached by at least one pair (A[r,u], B[u,j]); a touched column whose sum is 0.0 is
// still a candidate.  The value of column j is the reference's SparseMatrixMultiplier sum (implicit/nearest_neighbours.h):
//   s_j = ((0.0 + B[u_1,j]*A[r,u_1]) + B[u_2,j]*A[r,u_2]) + ...     over the entries u_1, u_2, ... of A[r] that reach j, IN
// A[r]'s STORED ORDER, every product and sum a separately rounded fp64 operation (-ffp-contract=off), so s_j is bitwise the
// reference's.  zero_own_columns (the reference's remove_own_likes) then sets s_c = 0.0 for every TOUCHED column c that is
// also a column of A[r]; the column stays a candidate.  Row r's output is the k best candidates under the total order
// (score descending, column descending), written in that order; entries past counts[r] = min(k, touched) hold id -1 and
// score -inf.  There are no float atomics and every sum has the one order above: equal inputs give bitwise equal outputs.
//
// Accumulation.  One wavefront per row walks A[r] entry by entry (a wave-uniform loop; the next 64 entries and their B row
// bounds are loaded together, one per lane, KnnEntries); its 64 lanes take B[u]'s entries 64 at a time.  B has no repeated column within a row (imp_spmat_create checks), so the lanes of one step never add to
// the same column, and the steps of one wave reach memory in program order (LDS: in-order per wave; global: a workgroup-scope
// fence between steps).  That fixes the order of every column's sum to A[r]'s order without atomics on the values.
//   pass 1, knn_hash_kernel: every row, one 64-lane workgroup each, accumulates into an open-addressing table of kHashSlots
//     (column id, fp64 sum) pairs in LDS (24 KiB: six rows per CU).  A new column claims its slot with an int32 CAS on the
//     id (only the slot, never a value, depends on that race).  A row whose touched count passes kHashLimit stops and is
//     appended to the overflow list.
//   pass 2, knn_dense_kernel: a fixed set of workers (one wavefront each) takes the overflow rows; each worker owns a dense
//     fp64 accumulator of C columns in global memory, kept at a sentinel NaN between rows, and a list of the columns it
//     touched (its candidate list; only those are reset afterwards).
// Selection (both passes).  The candidates are scanned 64 at a time; a sorted list of up to 64*R (score, column) pairs lives
// in registers, lane l holding positions l, l+64, ...; each candidate that beats the list's last kept entry is inserted
// with one ballot per register and a shift by shuffles.  k above 64*R runs further rounds, each over the candidates strictly
// below the last entry written, until k entries are written or the candidates run out -- exact for any k (R = 4 there).
// (Not on select_ops.h: its keys carry fp32 scores, these scores are double and never leave registers; golden files pin the order.)
#include <cfloat>
#include <cstring>
#include <vector>

#include "common.h"

struct imp_spmat {
  int32_t rows = 0, cols = 0;
  int64_t nnz = 0;
  bool unique_cols = true;  // no column repeated within a row (required of the right operand B)
  imp::DeviceArray<int64_t> indptr;
  imp::DeviceArray<int32_t> indices;
  imp::DeviceArray<double> data;
};

namespace imp {

constexpr int kHashSlots = 2048;
constexpr int kHashLimit = 1536;  // touched columns beyond which a row leaves the LDS table for the dense pass
constexpr uint64_t kUntouched = 0x7ff4deadbeef0001ull;  // signalling-NaN payload: no sum of products produces it

struct KnnArgs {
  const int64_t *__restrict__ a_ptr;
  const int32_t *__restrict__ a_idx;
  const double *__restrict__ a_val;
  const int64_t *__restrict__ b_ptr;
  const int32_t *__restrict__ b_idx;
  const double *__restrict__ b_val;
  int32_t *__restrict__ ids;   // [rows of this chunk x k]
  double *__restrict__ scores;
  int32_t *__restrict__ counts;
  int32_t *__restrict__ over;  // overflow rows (chunk-relative), over_n their count
  int32_t *__restrict__ over_n;
  double *__restrict__ acc;     // [workers x C] dense accumulators (pass 2)
  int32_t *__restrict__ touched;  // [workers x C]
  int32_t row0, nrows, k, zero_own;
  int32_t C, workers;
};

__device__ __forceinline__ bool knn_better(double s1, int c1, double s2, int c2) {
  return s1 > s2 || (s1 == s2 && c1 > c2);
}

__device__ __forceinline__ void knn_step_fence_lds() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ void knn_step_fence_global() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// Sorted list of up to 64*R (score, column) pairs, best first; lane l holds positions l + 64 i in s[i], c[i].
template <int R> struct TopList {
  double s[R];
  int c[R];
  __device__ void clear() {
#pragma unroll
    for (int i = 0; i < R; ++i) s[i] = -__builtin_inf(), c[i] = -1;
  }
  // entry at position p (wave-uniform) in every lane
  __device__ void at(int p, double &sp, int &cp) const {
    const int i = p >> 6, l = p & 63;
    double v = s[0];
    int w = c[0];
#pragma unroll
    for (int q = 1; q < R; ++q)
      if (q == i) v = s[q], w = c[q];
    sp = __shfl(v, l);
    cp = __shfl(w, l);
  }
  // inserts (x, y), which is known to beat the entry at position cap - 1
  __device__ void insert(double x, int y) {
    const int lane = threadIdx.x & 63;
    int pos = 0;
#pragma unroll
    for (int i = 0; i < R; ++i) pos += __popcll(__ballot(knn_better(s[i], c[i], x, y)));
    double ps[R];
    int pc[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      ps[i] = __shfl(s[i], (lane + 63) & 63);
      pc[i] = __shfl(c[i], (lane + 63) & 63);
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
      // the predecessor of position 64 i + lane: lane - 1 of the same register, or lane 63 of the register before
      double prev_s = ps[i];
      int prev_c = pc[i];
      if (lane == 0) {
        prev_s = i > 0 ? ps[i > 0 ? i - 1 : 0] : -__builtin_inf();
        prev_c = i > 0 ? pc[i > 0 ? i - 1 : 0] : -1;
      }
      const int e = 64 * i + lane;
      if (e == pos) s[i] = x, c[i] = y;
      else if (e > pos) s[i] = prev_s, c[i] = prev_c;
    }
  }
};

// Selects and writes row `row`'s output from the candidate set: cand(t, s, c) yields candidate t of n (valid = c >= 0).
template <int R, typename Cand>
__device__ void knn_select(const KnnArgs &a, int row, int64_t n, Cand cand) {
  const int lane = threadIdx.x & 63;
  int32_t *ids = a.ids + (size_t)row * a.k;
  double *scores = a.scores + (size_t)row * a.k;
  int written = 0;
  double last_s = __builtin_inf();
  int last_c = INT32_MAX;
  bool first = true;
  while (written < a.k) {
    const int cap = min(64 * R, a.k - written);
    TopList<R> L;
    L.clear();
    int have = 0;
    for (int64_t t0 = 0; t0 < n; t0 += 64) {
      double x = 0.0;
      int y = -1;
      if (t0 + lane < n) cand(t0 + lane, x, y);
      bool ok = y >= 0 && (first || knn_better(last_s, last_c, x, y));
      double ks;
      int kc;
      L.at(cap - 1, ks, kc);
      uint64_t m = __ballot(ok && knn_better(x, y, ks, kc));
      while (m) {
        const int src = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        const double xs = __shfl(x, src);
        const int yc = __shfl(y, src);
        L.at(cap - 1, ks, kc);
        if (!knn_better(xs, yc, ks, kc)) continue;
        L.insert(xs, yc);
        ++have;
      }
    }
    const int got = min(have, cap);
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int e = 64 * i + lane;
      if (e < got) ids[written + e] = L.c[i], scores[written + e] = L.s[i];
    }
    if (got > 0) L.at(got - 1, last_s, last_c);
    written += got;
    first = false;
    if (got < cap) break;
  }
  for (int e = written + lane; e < a.k; e += 64) ids[e] = -1, scores[e] = -__builtin_inf();
  if (lane == 0) a.counts[row] = written;
}

// The next 64 entries of A[r] (from pb), one per lane, with their B row bounds: loaded together instead of one dependent
// chain (A entry -> B offsets) per step
struct KnnEntries {
  double w;
  long long q0, q1;
  int n;
  __device__ KnnEntries(const KnnArgs &a, int64_t pb, int64_t p1) {
    const int64_t p = pb + (threadIdx.x & 63);
    n = (int)min((int64_t)64, p1 - pb);
    w = 0.0, q0 = q1 = 0;
    if (p < p1) {
      const int u = a.a_idx[p];
      w = a.a_val[p];
      q0 = a.b_ptr[u];
      q1 = a.b_ptr[u + 1];
    }
  }
  __device__ void get(int e, double &we, int64_t &b0, int64_t &b1) const {
    we = __shfl(w, e);
    b0 = __shfl(q0, e);
    b1 = __shfl(q1, e);
  }
};

__device__ __forceinline__ int knn_hash(int j) { return (int)(((uint32_t)j * 2654435761u) >> 21) & (kHashSlots - 1); }

template <int R>
__global__ __launch_bounds__(64) void knn_hash_kernel(KnnArgs a) {
  __shared__ int keys[kHashSlots];
  __shared__ double vals[kHashSlots];
  const int lane = threadIdx.x;
  const int row = blockIdx.x;  // chunk-relative
  const int64_t ar = (int64_t)a.row0 + row;
  for (int t = lane; t < kHashSlots; t += 64) keys[t] = -1;
  knn_step_fence_lds();
  const int64_t p0 = a.a_ptr[ar], p1 = a.a_ptr[ar + 1];
  int distinct = 0;
  for (int64_t pb = p0; pb < p1; pb += 64) {
    KnnEntries E(a, pb, p1);
    for (int e = 0; e < E.n; ++e) {
      double w;
      int64_t q0, q1;
      E.get(e, w, q0, q1);
      for (int64_t qb = q0; qb < q1; qb += 64) {
        const int64_t q = qb + lane;
        bool fresh = false;
        if (q < q1) {
          const int j = a.b_idx[q];
          const double v = a.b_val[q] * w;
          int slot = knn_hash(j);
          while (true) {
            int key = keys[slot];
            if (key == -1) {
              key = atomicCAS(&keys[slot], -1, j);
              if (key == -1) {
                fresh = true;
                break;
              }
            }
            if (key == j) break;
            slot = (slot + 1) & (kHashSlots - 1);
          }
          vals[slot] = fresh ? 0.0 + v : vals[slot] + v;
        }
        distinct += __popcll(__ballot(fresh));
        knn_step_fence_lds();
        if (distinct > kHashLimit) {
          if (lane == 0) a.over[atomicAdd(a.over_n, 1)] = row;
          return;
        }
      }
    }
  }
  if (a.zero_own) {
    for (int64_t p = p0 + lane; p < p1; p += 64) {
      const int c = a.a_idx[p];
      int slot = knn_hash(c);
      while (true) {
        const int key = keys[slot];
        if (key == -1) break;
        if (key == c) {
          vals[slot] = 0.0;
          break;
        }
        slot = (slot + 1) & (kHashSlots - 1);
      }
    }
    knn_step_fence_lds();
  }
  knn_select<R>(a, row, kHashSlots, [&](int64_t t, double &s, int &c) {
    c = keys[t];
    s = vals[t];
  });
}

__device__ __forceinline__ bool knn_untouched(double v) { return (uint64_t)__double_as_longlong(v) == kUntouched; }

template <int R>
__global__ __launch_bounds__(64) void knn_dense_kernel(KnnArgs a) {
  const int lane = threadIdx.x;
  double *acc = a.acc + (size_t)blockIdx.x * a.C;
  int32_t *touched = a.touched + (size_t)blockIdx.x * a.C;
  const int n_over = *a.over_n;
  for (int i = blockIdx.x; i < n_over; i += a.workers) {
    const int row = a.over[i];
    const int64_t ar = (int64_t)a.row0 + row;
    const int64_t p0 = a.a_ptr[ar], p1 = a.a_ptr[ar + 1];
    int n = 0;
    for (int64_t pb = p0; pb < p1; pb += 64) {
      KnnEntries E(a, pb, p1);
      for (int e = 0; e < E.n; ++e) {
        double w;
        int64_t q0, q1;
        E.get(e, w, q0, q1);
        for (int64_t qb = q0; qb < q1; qb += 64) {
          const int64_t q = qb + lane;
          bool fresh = false;
          int j = 0;
          if (q < q1) {
            j = a.b_idx[q];
            const double v = a.b_val[q] * w;
            const double old = acc[j];
            fresh = knn_untouched(old);
            acc[j] = fresh ? 0.0 + v : old + v;
          }
          const uint64_t m = __ballot(fresh);
          if (fresh) touched[n + __popcll(m & ((1ull << lane) - 1))] = j;
          n += __popcll(m);
          knn_step_fence_global();
        }
      }
    }
    if (a.zero_own) {
      for (int64_t p = p0 + lane; p < p1; p += 64) {
        const int c = a.a_idx[p];
        if (!knn_untouched(acc[c])) acc[c] = 0.0;
      }
      knn_step_fence_global();
    }
    knn_select<R>(a, row, n, [&](int64_t t, double &s, int &c) {
      c = touched[t];
      s = acc[c];
    });
    knn_step_fence_global();
    for (int t = lane; t < n; t += 64) acc[touched[t]] = __longlong_as_double((long long)kUntouched);
    knn_step_fence_global();
  }
}

__global__ void knn_fill_untouched(double *acc, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) acc[i] = __longlong_as_double((long long)kUntouched);
}

}  // namespace imp

using namespace imp;

extern "C" int imp_spmat_create(int32_t rows, int32_t cols, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                                const double *data, imp_spmat **out) {
  return guarded([&] {
    if (!out) throw std::invalid_argument("spmat_create: NULL output handle");
    if (rows < 0 || cols < 0 || nnz < 0) throw std::invalid_argument("spmat_create: negative dimension");
    if (nnz > INT32_MAX) throw std::invalid_argument("spmat_create: more than 2^31-1 nonzeros is not supported");
    if (!indptr || (nnz && (!indices || !data))) throw std::invalid_argument("spmat_create: NULL array");
    if (indptr[0] != 0 || indptr[rows] != nnz) throw std::invalid_argument("spmat_create: indptr must run from 0 to nnz");
    bool unique = true;
    std::vector<int32_t> mark(cols, -1);
    for (int32_t r = 0; r < rows; ++r) {
      // checked before the row is read: an offset beyond nnz would lead the loop below past the end of indices
      if (indptr[r + 1] < indptr[r] || indptr[r + 1] > nnz)
        throw std::invalid_argument("spmat_create: indptr must be non-decreasing and end at nnz");
      for (int64_t p = indptr[r]; p < indptr[r + 1]; ++p) {
        const int32_t c = indices[p];
        if (c < 0 || c >= cols) throw std::invalid_argument("spmat_create: column id out of range");
        if (mark[c] == r) unique = false;
        mark[c] = r;
      }
    }
    auto m = std::make_unique<imp_spmat>();
    m->rows = rows, m->cols = cols, m->nnz = nnz, m->unique_cols = unique;
    m->indptr.upload(indptr, (size_t)rows + 1);
    m->indices.upload(indices, (size_t)nnz);
    m->data.upload(data, (size_t)nnz);
    sync();
    *out = m.release();
  });
}

extern "C" int imp_spmat_destroy(imp_spmat *m) {
  return guarded([&] { delete m; });
}

extern "C" int imp_sparse_topk_product(const imp_spmat *A, const imp_spmat *B, int k, int zero_own_columns, int32_t *ids,
                                       double *scores, int32_t *counts) {
  return guarded([&] {
    if (!A || !B || !counts || ((!ids || !scores) && A && A->rows > 0)) throw std::invalid_argument("sparse_topk_product: NULL argument");
    if (A->cols != B->rows) throw std::invalid_argument("sparse_topk_product: A.cols must equal B.rows");
    if (k < 1) throw std::invalid_argument("sparse_topk_product: k must be >= 1");
    if (A->nnz > INT32_MAX || B->nnz > INT32_MAX)
      throw std::invalid_argument("sparse_topk_product: more than 2^31-1 nonzeros is not supported");
    if (zero_own_columns && A->cols != B->cols)
      throw std::invalid_argument("sparse_topk_product: zero_own_columns needs A.cols == B.cols");
    if (!B->unique_cols) throw std::invalid_argument("sparse_topk_product: B repeats a column within a row (sum duplicates first)");
    if (A->rows == 0) return;
    const int C = B->cols;
    Context &cx = ctx();
    // rows per launch: the device output of a chunk stays below ~1 GiB whatever k is
    const int64_t per_row = (int64_t)k * 12 + 8;
    const int32_t chunk = (int32_t)std::max<int64_t>(1, std::min<int64_t>(A->rows, ((int64_t)1 << 30) / per_row));
    DeviceArray<int32_t> d_ids, d_counts, d_over;
    DeviceArray<double> d_scores;
    d_ids.alloc((size_t)chunk * k);
    d_scores.alloc((size_t)chunk * k);
    d_counts.alloc((size_t)chunk + 1);
    d_over.alloc((size_t)chunk);
    // dense workers: as many as fit ~1.5 GiB of accumulators, at most 4 per CU
    const int workers = (int)std::max<int64_t>(
        1, std::min<int64_t>((int64_t)cx.num_cus * 4, ((int64_t)3 << 29) / std::max<int64_t>(1, (int64_t)C * 12)));
    if (cx.knn_acc.size < (size_t)workers * C || cx.knn_cols != C) {
      cx.knn_acc.alloc(std::max<size_t>(1, (size_t)workers * C));
      cx.knn_touched.alloc(std::max<size_t>(1, (size_t)workers * C));
      cx.knn_cols = C;
      const size_t n = cx.knn_acc.size;
      hipLaunchKernelGGL(knn_fill_untouched, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream(), cx.knn_acc.data(), n);
      IMP_CHECK_HIP(hipGetLastError());
    }
    KnnArgs a{A->indptr.data(), A->indices.data(), A->data.data(), B->indptr.data(), B->indices.data(), B->data.data(),
              d_ids.data(), d_scores.data(), d_counts.data(), d_over.data(), d_counts.data() + chunk, cx.knn_acc.data(),
              cx.knn_touched.data(), 0, 0, k, zero_own_columns ? 1 : 0, C, workers};
    for (int32_t r0 = 0; r0 < A->rows; r0 += chunk) {
      a.row0 = r0;
      a.nrows = std::min(chunk, A->rows - r0);
      IMP_CHECK_HIP(hipMemsetAsync(a.over_n, 0, sizeof(int32_t), stream()));
      {
        IMP_PROF("knn_hash");
        if (k <= 64) hipLaunchKernelGGL(knn_hash_kernel<1>, dim3(a.nrows), dim3(64), 0, stream(), a);
        else hipLaunchKernelGGL(knn_hash_kernel<4>, dim3(a.nrows), dim3(64), 0, stream(), a);
        IMP_CHECK_HIP(hipGetLastError());
      }
      {
        IMP_PROF("knn_dense");
        if (k <= 64) hipLaunchKernelGGL(knn_dense_kernel<1>, dim3(workers), dim3(64), 0, stream(), a);
        else hipLaunchKernelGGL(knn_dense_kernel<4>, dim3(workers), dim3(64), 0, stream(), a);
        IMP_CHECK_HIP(hipGetLastError());
      }
      IMP_CHECK_HIP(hipMemcpyAsync(ids + (size_t)r0 * k, a.ids, (size_t)a.nrows * k * sizeof(int32_t), hipMemcpyDeviceToHost, stream()));
      IMP_CHECK_HIP(hipMemcpyAsync(scores + (size_t)r0 * k, a.scores, (size_t)a.nrows * k * sizeof(double), hipMemcpyDeviceToHost, stream()));
      IMP_CHECK_HIP(hipMemcpyAsync(counts + r0, a.counts, (size_t)a.nrows * sizeof(int32_t), hipMemcpyDeviceToHost, stream()));
      sync();
    }
  });
}
