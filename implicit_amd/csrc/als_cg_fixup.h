// One row of the fp32 fix-up solver of the f = 64 / 128 CG path (als_cg_fixup.hip has the kernel and its producers), as a device
// function: the stand-alone kernel runs it, and so does the chain of the two 1024-thread classes at its head (als_cg_qf.hip).
// Arithmetic contract: the oracle's CG (implicit/cpu/_als.pyx:152-248).
#ifndef IMPLICIT_AMD_CSRC_ALS_CG_FIXUP_H_
#define IMPLICIT_AMD_CSRC_ALS_CG_FIXUP_H_

#include "als_qtile.h"
#include "common.h"
#include "wave_ops.h"

namespace imp {

// One wavefront solves row u, everything streamed in fp32: lane l owns the FC = F / 64 consecutive factors FC l ..; a nonzero is
// one coalesced row read, one wave-wide dot product, one axpy (four nonzeros' reads in flight); the gramian comes from global
// memory (L2) row by row with the operand broadcast from `vec`, F floats of LDS private to the wavefront.  No workgroup barrier.
template <int F, typename ST>
__device__ __forceinline__ void cg_fixup_row(float *vec, int lane, int u, const int32_t *__restrict__ indptr,
                                             const int32_t *__restrict__ indices, const float *__restrict__ data, ST *__restrict__ X,
                                             const ST *__restrict__ Y, const float *__restrict__ A0, int cg_steps) {
  constexpr int FC = F / 64, U = 4;
  auto load_vec = [&](const ST *row, float (&v)[FC]) {
#pragma unroll
    for (int c = 0; c < FC; ++c) v[c] = load1(row + FC * lane + c);
  };
  // acc = sign * A0 v + sum_k w_k y_k,  w_k = FIRST ? c+ - (|c|-1) y_k.v : (|c|-1) y_k.v
  auto apply = [&](bool first, int rb, int re, const float (&v)[FC], float (&acc)[FC]) {
#pragma unroll
    for (int c = 0; c < FC; ++c) vec[FC * lane + c] = v[c];  // wave-private: no barrier
#pragma unroll
    for (int c = 0; c < FC; ++c) acc[c] = 0.f;
    for (int j = 0; j < F; ++j) {
      const float vj = vec[j];
#pragma unroll
      for (int c = 0; c < FC; ++c) acc[c] = fmaf(A0[(size_t)j * F + FC * lane + c], vj, acc[c]);
    }
    if (first) {
#pragma unroll
      for (int c = 0; c < FC; ++c) acc[c] = -acc[c];
    }
    for (int k0 = rb; k0 < re; k0 += U) {
      float conf[U], y[U][FC];
#pragma unroll
      for (int q = 0; q < U; ++q) {
        const int k = min(k0 + q, re - 1);
        conf[q] = data[k];
        load_vec(Y + (size_t)indices[k] * F, y[q]);
      }
#pragma unroll
      for (int q = 0; q < U; ++q) {
        if (k0 + q < re) {  // wave-uniform
          const float d = wave_allsum(dot_local<FC>(y[q], v));
          const float cm1 = fabsf(conf[q]) - 1.f;
          const float w = first ? fmaxf(conf[q], 0.f) - cm1 * d : cm1 * d;
#pragma unroll
          for (int c = 0; c < FC; ++c) acc[c] = fmaf(w, y[q][c], acc[c]);
        }
      }
    }
  };
  const int rb = indptr[u], re = indptr[u + 1];
  ST *xrow = X + (size_t)u * F;
  float x[FC], r[FC], p[FC], Ap[FC];
  load_vec(xrow, x);
  apply(true, rb, re, x, r);
#pragma unroll
  for (int c = 0; c < FC; ++c) p[c] = r[c];
  float rsold = wave_allsum(dot_local<FC>(r, r));
  if (rsold < 1e-20f) return;  // x untouched (_als.pyx:206)
  for (int it = 0; it < cg_steps; ++it) {
    apply(false, rb, re, p, Ap);
    const float alpha = rsold / wave_allsum(dot_local<FC>(p, Ap));
#pragma unroll
    for (int c = 0; c < FC; ++c) {
      x[c] = fmaf(alpha, p[c], x[c]);
      r[c] = fmaf(-alpha, Ap[c], r[c]);
    }
    const float rsnew = wave_allsum(dot_local<FC>(r, r));
    if (rsnew < 1e-20f) break;
    const float beta = rsnew / rsold;
#pragma unroll
    for (int c = 0; c < FC; ++c) p[c] = fmaf(beta, p[c], r[c]);
    rsold = rsnew;
  }
#pragma unroll
  for (int c = 0; c < FC; ++c) store1(xrow + FC * lane + c, x[c]);
}

}  // namespace imp

#endif  // IMPLICIT_AMD_CSRC_ALS_CG_FIXUP_H_
