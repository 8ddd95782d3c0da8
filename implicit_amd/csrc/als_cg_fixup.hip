// Fix-up solver of the f = 64 / 128 CG path: rows a fast kernel could not finish are re-solved in fp32, one wavefront per row.
// Arithmetic contract: the oracle's CG (implicit/cpu/_als.pyx:152-248).
#include <type_traits>

#include "als_cg_fixup.h"
#include "als_qtile.h"
#include "common.h"

namespace imp {

// ---- fix-up of the rows another kernel left unsolved ---------------------------------------------------------------------
// Producer: the normal-matrix kernels (als_cg_nm.hip: a row whose fp16-split operands left the fp16 range; until round 5 also a
// cluster of workgroups whose exchange was lost -- those kernels are gone).  One wavefront per listed row (cg_fixup_row,
// als_cg_fixup.h): the oracle's CG step by step (_als.pyx:179-244); only the summation order differs from the producers'.
// Slow (a millisecond for a 4096-nonzero row) and never expected to have work; `total` (host-mapped, imp_solver_fixup_rows)
// counts the rows it has re-solved.
template <int F, typename ST>
__global__ __launch_bounds__(256) void als_cg_fault_fixup_kernel(const unsigned *__restrict__ fault_count,
                                                                 const unsigned *__restrict__ fault_rows, int capacity,
                                                                 const int32_t *__restrict__ indptr,
                                                                 const int32_t *__restrict__ indices,
                                                                 const float *__restrict__ data, ST *__restrict__ X,
                                                                 const ST *__restrict__ Y, const float *__restrict__ A0, int cg_steps,
                                                                 unsigned long long *total) {
  constexpr int WAVES = 4;
  __shared__ float vecs[WAVES][F];
  const int n = min((int)fault_count[0], capacity);
  if (n == 0) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_fetch_add(total, (unsigned long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = blockIdx.x * WAVES + wave; i < n; i += gridDim.x * WAVES)
    cg_fixup_row<F, ST>(vecs[wave], lane, (int)fault_rows[i], indptr, indices, data, X, Y, A0, cg_steps);
}

// host-mapped counter of the rows the fix-up kernel has re-solved on this device (imp_solver_fixup_rows)
unsigned long long *fixup_total() {
  auto &c = ctx();
  if (!c.fixup_total) {
    IMP_CHECK_HIP(hipHostMalloc(reinterpret_cast<void **>(&c.fixup_total), sizeof(unsigned long long), hipHostMallocMapped));
    *c.fixup_total = 0ull;
  }
  return c.fixup_total;
}

// queued behind the kernels that fill the list; normally reads a zero and exits
template <int F, typename T>
void launch_cg_fixup(const unsigned *count, const unsigned *rows, int capacity, const imp_csr *C, T *X, const T *Y, const float *A0,
                     int cg_steps) {
  if (capacity <= 0) return;
  IMP_PROF("als_cg_fixup");
  als_cg_fault_fixup_kernel<F, T><<<std::min((capacity + 3) / 4, ctx().num_cus * 2), 256, 0, stream()>>>(
      count, rows, capacity, C->indptr.data(), C->indices.data(), C->data.data(), X, Y, A0, cg_steps, fixup_total());
  IMP_CHECK_HIP(hipGetLastError());
}
template void launch_cg_fixup<64, float>(const unsigned *, const unsigned *, int, const imp_csr *, float *, const float *, const float *, int);
template void launch_cg_fixup<128, float>(const unsigned *, const unsigned *, int, const imp_csr *, float *, const float *, const float *, int);
template void launch_cg_fixup<64, __half>(const unsigned *, const unsigned *, int, const imp_csr *, __half *, const __half *, const float *, int);
template void launch_cg_fixup<128, __half>(const unsigned *, const unsigned *, int, const imp_csr *, __half *, const __half *, const float *, int);


}  // namespace imp
