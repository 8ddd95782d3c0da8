// The host side the two sampled pairwise trainers share (imp_bpr_update, bpr.hip; imp_warp_update, warp.hip): the lane rule
// with its override, the id pre-pass and the common body of the two entry points.  sgd_group.h declares all three.
//
// Every id an update kernel turns into an address is checked on the device first (pair_check_kernel): an id outside its
// matrix returns IMP_OUT_OF_RANGE with nothing launched -- an out-of-bounds write is a device fault.
#include <cstdlib>
#include <string>

#include "common.h"
#include "sgd_group.h"

namespace imp {

// The pre-pass: 0 <= userids < x_rows, 0 <= itemids < y_rows, 0 <= indptr <= nnz.  Violations OR bits 1 / 2 / 4 into *bad.
// The first `quads` x 4 ids are read as int4 (16-byte aligned arrays), the rest one by one.
__global__ __launch_bounds__(256) void pair_check_kernel(const int32_t *__restrict__ userids, const int32_t *__restrict__ itemids,
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

int pair_group_lanes(int C) {
  if (const char *e = std::getenv("IMP_BPR_LANES")) {
    const int g = std::atoi(e);
    if ((g == 16 || g == 32 || g == 64) && C <= 16 * g) return g;
  }
  return group_lanes(C);
}

void check_pair_ids(const char *who, const char *prof, const imp_intvector *userids, const imp_intvector *itemids,
                    const imp_intvector *indptr, size_t x_rows, size_t y_rows, unsigned long long *bad_word) {
  const int64_t nnz = (int64_t)userids->size;
  {
    IMP_PROF(prof);
    const int64_t work = std::max(nnz / 4, (int64_t)indptr->size);
    const int grid = (int)std::min<int64_t>((work + 255) / 256, ctx().num_cus * 8);
    const bool aligned = ((uintptr_t)userids->v.data() | (uintptr_t)itemids->v.data()) % 16 == 0;
    pair_check_kernel<<<grid, 256, 0, stream()>>>(userids->v.data(), itemids->v.data(), nnz, aligned ? nnz / 4 : 0, indptr->v.data(),
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

void pair_update(const char *who, const char *check_prof, const char *prof, const imp_intvector *userids,
                 const imp_intvector *itemids, const imp_intvector *indptr, imp_matrix *X, imp_matrix *Y, int64_t samples,
                 int64_t *count0, int64_t *count1, const PairLaunch &launch) {
  const std::string w(who);
  if (!userids || !itemids || !indptr || !X || !Y || !count0 || !count1) throw std::invalid_argument(w + ": NULL argument");
  if (X->cols != Y->cols) throw std::invalid_argument("X and Y should have the same number of columns");
  if (X->cols < 2 || X->cols > 1024)
    throw std::invalid_argument(w + ": factor matrices need 2 .. 1024 columns (factors + 1 for the item bias)");
  if (X->itemsize != 4 || Y->itemsize != 4) throw std::invalid_argument(w + ": factor matrices must be float32");
  if (userids->size != itemids->size) throw std::invalid_argument("userids and itemids should have same number of elements");
  if (indptr->size != X->rows + 1) throw std::invalid_argument(w + ": indptr must have X.rows + 1 entries");
  const int64_t nnz = (int64_t)userids->size;
  if (nnz > INT32_MAX) throw std::invalid_argument(w + ": more than 2^31 - 1 nonzeros");
  const int64_t n = samples < 0 ? nnz : samples;
  *count0 = *count1 = 0;
  if (nnz == 0 || n == 0) return;

  unsigned long long *stats = ctx().pair_stats.reserve(3);
  IMP_CHECK_HIP(hipMemsetAsync(stats, 0, 3 * sizeof(unsigned long long), stream()));
  check_pair_ids(who, check_prof, userids, itemids, indptr, X->rows, Y->rows, stats + 2);

  {
    IMP_PROF(prof);
    const int G = pair_group_lanes((int)X->cols);
    const int cap = ctx().num_cus * 8;  // 8 workgroups of 4 waves per CU: the most the CU holds
    // the cap on concurrent samples (sgd_group.h); it holds for WARP's larger steps too: DESIGN 4.15
    const int64_t in_flight = hogwild_in_flight(n, X->rows, Y->rows);
    launch(G, (int)std::min<int64_t>((in_flight * G + 255) / 256, cap), n, stats);
    IMP_CHECK_HIP(hipGetLastError());
  }
  unsigned long long h[2];
  IMP_CHECK_HIP(hipMemcpyAsync(h, stats, sizeof(h), hipMemcpyDeviceToHost, stream()));
  sync();  // synchronous in deferred mode too: the counts are the result
  *count0 = (int64_t)h[0];
  *count1 = (int64_t)h[1];
}

}  // namespace imp
