// Zero-padded systems: a half sweep at a factor count f that has no kernels of its own runs on those of a wider F.
//
// CG rides F = 64 / 128 / 256 for every other f < 256 (als_cg.hip), Cholesky F = 128 for 64 < f < 128 (als_cholesky.hip).  Y, the
// solved rows of X and the gramian are copied with F columns, the new columns zero, the gramian extended by a unit diagonal
// block.  The padded system is block diagonal: its solution is the original one followed by zeros.  For CG that is exact step by
// step: residual, search direction and iterate stay zero in the padded components (b = 0, x0 = 0 there) and every dot product
// only gains exact zeros.  Cost: one padded copy of Y and of the solved rows of X in, the rows of X out -- (R_y + 2 R_x)(f + F)
// 4 bytes per half sweep, ~0.2 ms at configs[2] -- and the workspaces (PaddedSystem, common.h).
#include "common.h"

namespace imp {

__global__ void unpad_rows_kernel(const float *__restrict__ src, float *__restrict__ dst, size_t rows, int f, int F) {
  const size_t n = rows * (size_t)f;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i / f;
    dst[i] = src[r * F + (i - r * f)];
  }
}
// *same = 1 iff the f x f gramian of this call equals, bit for bit, the top-left block of the padded gramian of the previous
// one (single workgroup; the flag starts at 1 and any differing element clears it)
__global__ void pad_check_kernel(const float *__restrict__ gram, const float *__restrict__ padded, int f, int F, int *same) {
  if (threadIdx.x == 0) *same = 1;
  __syncthreads();
  bool differ = false;
  for (int i = threadIdx.x; i < f * f; i += blockDim.x) {
    const int r = i / f, c = i - r * f;
    differ |= __float_as_uint(gram[i]) != __float_as_uint(padded[(size_t)r * F + c]);
  }
  if (differ) *same = 0;
}
__global__ void pad_gram_kernel(const float *__restrict__ src, float *__restrict__ dst, int f, int F) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < F * F; i += gridDim.x * blockDim.x) {
    const int r = i / F, c = i - r * F;
    dst[i] = (r < f && c < f) ? src[r * f + c] : (r == c ? 1.f : 0.f);
  }
}

static int pad_grid(size_t n) { return (int)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, (size_t)ctx().num_cus * 16)); }

PaddedViews pad_in(const imp_matrix *X, const imp_matrix *Y, const imp_matrix *YtY, size_t rows_of_X, int F, bool reuse_y) {
  const int f = (int)X->cols;
  PaddedSystem &p = ctx().pad;
  const size_t rx = rows_of_X, ry = Y->rows;
  p.x.reserve(rx * F);
  // a copy that may not be re-used, or that goes with its buffer, is forgotten (before the reserve: freeing the buffer reports a
  // write to that memory)
  if (!reuse_y || p.y.size < ry * F) p.y_key.drop();
  p.y.reserve(ry * F);
  p.gram.reserve((size_t)F * F);
  {
    IMP_PROF("pad_factors");
    // The padded copy of Y is re-used when this call solves against the SAME matrix under the SAME gramian as the previous
    // one -- the K row chunks of a sharded half sweep (4 redundant copies of a 10 M-row replica otherwise).  Same memory, not
    // written through the library since (y_key), shape and factor counts are checked here; "same contents" is decided on the
    // device, with no host wait, through the gramian:
    // whoever changes Y recomputes YtY (the solve is meaningless otherwise), so a gramian equal bit for bit to the one the copy
    // was made under vouches for it.  The flag is read by the pad kernel itself, which then returns at once.
    const int *skip = nullptr;
    if (ry && p.y_key.made_from(Y) && p.y_rows == ry && p.y_f == f && p.y_F == F) {
      IMP_PROF_NESTED("padded_y_check");  // one count per call that found a kept copy to vouch for: what the cache tests read
      skip = p.same.reserve(1);
      pad_check_kernel<<<1, 1024, 0, stream()>>>(YtY->f32(), p.gram.data(), f, F, p.same.data());
    }
    if (ry) pad_rows(pad_grid(ry * F), Y->f32(), p.y.data(), ry, f, F, skip);
    // (no copy is kept of memory whose writes the library does not see: binding to such a matrix binds to nothing)
    if (reuse_y) p.y_key.bind(Y), p.y_rows = ry, p.y_f = f, p.y_F = F;
    if (rx) pad_rows(pad_grid(rx * F), X->f32(), p.x.data(), rx, f, F);
    pad_gram_kernel<<<pad_grid((size_t)F * F), 256, 0, stream()>>>(YtY->f32(), p.gram.data(), f, F);
    IMP_CHECK_HIP(hipGetLastError());
  }
  return {imp_matrix(rx, F, 4, p.x.storage), imp_matrix(ry, F, 4, p.y.storage), imp_matrix(F, F, 4, p.gram.storage)};
}

void pad_out(imp_matrix *X, size_t rows_of_X, int F) {
  const int f = (int)X->cols;
  IMP_PROF("unpad_factors");
  if (rows_of_X) unpad_rows_kernel<<<pad_grid(rows_of_X * f), 256, 0, stream()>>>(ctx().pad.x.data(), X->mut_rows<float>(0, rows_of_X), rows_of_X, f, F);
  IMP_CHECK_HIP(hipGetLastError());
}

}  // namespace imp
