// K2b: iALS++ block-subspace half sweep (Rendle, Krichene, Zhang, Koren 2021).  No reference counterpart.
//
// A row's system is A x = b, A = G + reg I + sum_j w_j y_j y_j^T, b = sum_j c+_j y_j (G the UNregularised gramian, w = |c| - 1,
// c+ = max(c, 0): the matrix of the Cholesky half sweep, als_cholesky.hip).  Instead of anything f x f per row, x is improved one
// block S of k coordinates at a time by an exact Newton step in that block, with the row's predictions p_j = x . y_j kept up to date:
//   g = (G x)_S + reg x_S + sum_j (w_j p_j - c+_j) y_j[S],   H = G_SS + reg I + sum_j w_j y_j[S] y_j[S]^T,
//   delta = -H^-1 g (Cholesky of k x k),   x_S += delta,   p_j += delta . y_j[S].
// K = 8, 16 or 32 is the instantiated block width; a narrower (or ragged last) block of kb < K coordinates runs with the padding
// made a unit diagonal and zero gradient: its delta is zero and is never stored.
//
// The sparse part of H is a SYRK over the gathered slices: v_mfma_f32_32x32x2_f32, two nonzeros per instruction, lane
// (r = l & 31, h = l >> 5) loads y_j[s0 + r] of nonzero 2 q + h -- at K = 32 one 128-byte segment per nonzero -- and feeds
// w y as the A operand and y as the B operand (exact fp32 products).  K = 8 and 16 run the same instruction with the lanes
// r >= K supplying zeros (32- and 64-byte gathers; three quarters / half of the matrix pipe idle): kept for correctness.  The
// gradient's sparse part is one FMA per lane on the same registers.  (G x)_S reads the block's k rows of G from L2.  The k x k
// system is solved by one wavefront in registers (lane i owns row i), the scheme of als_cholesky_wave_kernel.
//
// Predictions live in a workspace of nnz floats indexed by CSR position.  Rows of up to kCholLongRow nonzeros: one wavefront per
// row, longest first, the whole sweep in one kernel (every prediction is then read and written by the same lane).  Longer rows
// are cut into the segments of imp_csr::plan_chol and go block by block through three kernels -- per-segment partial (H, g); the
// fold in segment order with the solve; the prediction update -- every dependency a kernel boundary, no spin-wait, ticket or
// persistent workgroup.  Every reduction has a fixed order and there is no floating-point atomic: equal inputs, equal bits.
// The slices of a block are gathered twice per sweep (for H / g and for the prediction update); the second read finds them
// in L2.  Keeping them in the LDS between the two is future work.
#include "common.h"
#include "wave_ops.h"

namespace imp {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kSubMaxF = 1024;
constexpr int kSubPartial = 17 * 64;  // floats per segment partial: the accumulator tile in register order, then g

// wave-private LDS: one wavefront writes, the same wavefront reads through other lanes
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// pred[t] (SET: =, else +=) sum_{r < n} v[r] * Y[indices[t]][s0 + r] for the nonzeros [rb, re): one lane per nonzero, each lane
// walks its own item row's slice left to right (whole 128-byte segments at n = 32)
template <bool SET>
__device__ __forceinline__ void predict_range(const int32_t *__restrict__ indices, const float *__restrict__ Y, float *pred, int rb,
                                              int re, int f, int s0, int n, const float *v, int lane) {
  const bool vec = ((f | s0 | n) & 3) == 0;
  for (int t = rb + lane; t < re; t += 64) {
    const float *y = Y + (size_t)indices[t] * f + s0;
    float acc = 0.f;
    if (vec) {
#pragma unroll 4
      for (int r = 0; r < n; r += 4) {
        const float4 y4 = *reinterpret_cast<const float4 *>(y + r);
        acc = fmaf(v[r], y4.x, acc);
        acc = fmaf(v[r + 1], y4.y, acc);
        acc = fmaf(v[r + 2], y4.z, acc);
        acc = fmaf(v[r + 3], y4.w, acc);
      }
    } else {
      for (int r = 0; r < n; ++r) acc = fmaf(v[r], y[r], acc);
    }
    pred[t] = SET ? acc : pred[t] + acc;
  }
}

// acc += sum_j w_j y_j[S] y_j[S]^T (MFMA C/D layout), gs = sum_j (w_j p_j - c+_j) y_j[s0 + r] in lanes r and r + 32, over the
// nonzeros [rb, re) in stored order
__device__ __forceinline__ void block_partial(const int32_t *__restrict__ indices, const float *__restrict__ data,
                                              const float *__restrict__ Y, const float *pred, int rb, int re, int f, int s0, int kb,
                                              int lane, f32x16 &acc, float &gs) {
  const int r = lane & 31, h = lane >> 5;
  const bool active = r < kb;
  const int yoff = s0 + (active ? r : 0);
  for (int k0 = rb; k0 < re; k0 += 64) {
    const int cnt = min(64, re - k0);
    const bool mine = lane < cnt;
    const int my_idx = indices[k0 + min(lane, cnt - 1)];
    const float c = mine ? data[k0 + lane] : 1.f;
    const float p = mine ? pred[k0 + lane] : 0.f;
    const float my_w = mine ? fabsf(c) - 1.f : 0.f;
    const float my_cf = mine ? my_w * p - fmaxf(c, 0.f) : 0.f;
    for (int t0 = 0; t0 < cnt; t0 += 8) {  // four k-steps = eight nonzeros per trip, their gathers in flight together
      float y[4], w[4], cf[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int t = t0 + 2 * q + h;
        const int tc = min(t, cnt - 1);
        const unsigned col = (unsigned)__shfl(my_idx, tc, 64);
        const float wv = __shfl(my_w, tc, 64), cv = __shfl(my_cf, tc, 64);
        w[q] = t < cnt ? wv : 0.f;
        cf[q] = t < cnt ? cv : 0.f;
        y[q] = active ? Y[(size_t)col * f + yoff] : 0.f;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[q] * y[q], y[q], acc, 0, 0, 0);
        gs = fmaf(cf[q], y[q], gs);
      }
    }
  }
  gs += __shfl_xor(gs, 32, 64);
}

// The Newton step of one block from its sparse parts (acc, gs): adds the gramian's part, solves, stores delta (zero in the
// padding) to dl[0 .. K) and adds it to xs[s0 .. s0 + kb).  xs: the row's x in wave-private LDS, Hs: K x (K + 1) floats of
// wave-private LDS.  false on a non-positive pivot (xs, dl untouched).
template <int K>
__device__ __forceinline__ bool solve_block(const f32x16 &acc, float gs, const float *__restrict__ G, float *xs, float *Hs, float *dl,
                                            int f, int s0, int kb, float reg, int lane) {
  constexpr int LD = K + 1;
  const int r = lane & 31, h = lane >> 5;
  // (G x)_S: row s0 + s of G against x, lanes strided over the row, one wave sum per row of the block
  // (eight rows at a time: their loads are independent and in flight together; one row after the other the block paid a
  // round trip to L2 per row, 32 in a row, which nothing covered)
  float gx = 0.f;
  for (int sb = 0; sb < kb; sb += 8) {
    float part[8];
    const float *grow[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      part[q] = 0.f;
      grow[q] = G + (size_t)(s0 + min(sb + q, kb - 1)) * f;  // beyond the block: the last row again, its sum unused
    }
    for (int i = lane; i < f; i += 64) {
      const float xi = xs[i];
#pragma unroll
      for (int q = 0; q < 8; ++q) part[q] = fmaf(grow[q][i], xi, part[q]);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float total = wave_allsum(part[q]);
      if (r == sb + q) gx = total;
    }
  }
  float b = (lane < kb) ? gs + gx + reg * xs[s0 + lane] : 0.f;  // lane i: g_i
  // sparse part of H: accumulator tile -> LDS image (C/D layout: column = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5))
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int i = (e & 3) + 8 * (e >> 2) + 4 * h;
    if (i < K && r < K) Hs[i * LD + r] = acc[e];
  }
  wave_lds_fence();
  // lane i owns row i: H = image + G_SS + reg I inside the block, the identity in the padding (and in the lanes beyond K)
  float A[K];
  const bool in = lane < kb;
  const float *gblock = G + (size_t)(s0 + (in ? lane : 0)) * f + s0;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    float a = lane == j ? 1.f : 0.f;
    if (in && j < kb) a = Hs[lane * LD + j] + gblock[j] + (lane == j ? reg : 0.f);
    A[j] = a;
  }
  // right-looking Cholesky in registers, the forward substitution riding along (als_cholesky_wave_kernel)
  bool ok = true;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float d = lane_bcast(A[k], k);
    if (!(d > 0.f)) ok = false;
    const float sd = sqrtf(d);
    const float lik = lane == k ? sd : A[k] / sd;
    A[k] = lik;
    const float zk = lane_bcast(b, k) / sd;
    b = lane == k ? zk : (lane > k ? fmaf(-lik, zk, b) : b);
#pragma unroll
    for (int j = k + 1; j < K; ++j) A[j] = fmaf(-lik, lane_bcast(lik, j), A[j]);
  }
  wave_lds_fence();  // the image may be rewritten by the next block only after every lane has read its row
  if (!ok) return false;
  // back substitution L^T s = z; lane i ends with s_i = (H^-1 g)_i
#pragma unroll
  for (int k = K - 1; k >= 0; --k) {
    float t = lane > k ? A[k] * b : 0.f;
    t = group_allsum<64>(t);
    const float sk = (lane_bcast(b, k) - t) / lane_bcast(A[k], k);
    if (lane == k) b = sk;
  }
  if (lane < K) dl[lane] = in ? -b : 0.f;
  if (in) xs[s0 + lane] += -b;
  wave_lds_fence();
  return true;
}

// ---- rows of <= kCholLongRow nonzeros: one wavefront per row, the whole call in one kernel ----------------------------------------
template <int K>
__global__ __launch_bounds__(256, 3) void subspace_wave_kernel(const int32_t *__restrict__ order, int first, int count,
                                                            const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                            const float *__restrict__ data, float *__restrict__ X,
                                                            const float *__restrict__ Y, const float *__restrict__ G, float *pred, int f,
                                                            float reg, int block, int sweeps, unsigned long long *failed_row) {
  __shared__ float xs_all[4][kSubMaxF];
  __shared__ float hs_all[4][K * (K + 1)];
  __shared__ float dl_all[4][K];
  const int lane = threadIdx.x & 63, wslot = threadIdx.x >> 6;
  float *xs = xs_all[wslot], *Hs = hs_all[wslot], *dl = dl_all[wslot];
  const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
  const int nwaves = (gridDim.x * blockDim.x) >> 6;
  for (int ri = wave; ri < count; ri += nwaves) {
    const int u = __builtin_amdgcn_readfirstlane(order[first + ri]);
    const int rb = __builtin_amdgcn_readfirstlane(indptr[u]), re = __builtin_amdgcn_readfirstlane(indptr[u + 1]);
    float *xrow = X + (size_t)u * f;
    for (int i = lane; i < f; i += 64) xs[i] = xrow[i];
    wave_lds_fence();
    predict_range<true>(indices, Y, pred, rb, re, f, 0, f, xs, lane);
    bool ok = true;
    for (int sw = 0; sw < sweeps && ok; ++sw)
      for (int s0 = 0; s0 < f && ok; s0 += block) {
        const int kb = min(block, f - s0);
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
        float gs = 0.f;
        block_partial(indices, data, Y, pred, rb, re, f, s0, kb, lane, acc, gs);
        ok = solve_block<K>(acc, gs, G, xs, Hs, dl, f, s0, kb, reg, lane);
        if (ok) predict_range<false>(indices, Y, pred, rb, re, f, s0, kb, dl, lane);
      }
    if (ok) {
      for (int i = lane; i < f; i += 64) xrow[i] = xs[i];
    } else if (lane == 0) {
      atomicMin(failed_row, (unsigned long long)u);
    }
    wave_lds_fence();
  }
}

// ---- rows of more than kCholLongRow nonzeros: segments of plan_chol, a kernel per dependency ---------------------------------------
// predictions of every segment's nonzeros from the stored x
__global__ __launch_bounds__(256) void subspace_long_predict_kernel(const LongPlanDev plan, const int32_t *__restrict__ indices,
                                                                    const float *__restrict__ X, const float *__restrict__ Y,
                                                                    float *pred, int f) {
  __shared__ float xs_all[4][kSubMaxF];
  const int lane = threadIdx.x & 63;
  float *xs = xs_all[threadIdx.x >> 6];
  const int sg = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
  if (sg >= plan.n_seg) return;
  const float *xrow = X + (size_t)plan.rows[plan.seg_row[sg]] * f;
  for (int i = lane; i < f; i += 64) xs[i] = xrow[i];
  wave_lds_fence();
  predict_range<true>(indices, Y, pred, plan.seg_begin[sg], plan.seg_end[sg], f, 0, f, xs, lane);
}

// one wavefront per segment: its part of the block's (H, g)
__global__ __launch_bounds__(256) void subspace_long_partial_kernel(const LongPlanDev plan, const int32_t *__restrict__ indices,
                                                                    const float *__restrict__ data, const float *__restrict__ Y,
                                                                    const float *pred, int f, int s0, int kb,
                                                                    const int *__restrict__ row_failed, float *__restrict__ partials) {
  const int lane = threadIdx.x & 63;
  const int sg = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
  if (sg >= plan.n_seg || row_failed[plan.seg_row[sg]]) return;
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  float gs = 0.f;
  block_partial(indices, data, Y, pred, plan.seg_begin[sg], plan.seg_end[sg], f, s0, kb, lane, acc, gs);
  float *out = partials + (size_t)sg * kSubPartial + lane;
#pragma unroll
  for (int e = 0; e < 16; ++e) out[e * 64] = acc[e];
  out[16 * 64] = gs;
}

// one wavefront per long row: the segments' parts summed in segment order, the block's Newton step, x_S stored, delta kept
template <int K>
__global__ __launch_bounds__(256) void subspace_long_solve_kernel(const LongPlanDev plan, float *__restrict__ X, const float *__restrict__ G,
                                                                  const float *__restrict__ partials, int f, int s0, int kb, float reg,
                                                                  int *row_failed, float *__restrict__ delta,
                                                                  unsigned long long *failed_row) {
  __shared__ float xs_all[4][kSubMaxF];
  __shared__ float hs_all[4][K * (K + 1)];
  __shared__ float dl_all[4][K];
  const int lane = threadIdx.x & 63, wslot = threadIdx.x >> 6;
  float *xs = xs_all[wslot], *Hs = hs_all[wslot], *dl = dl_all[wslot];
  const int li = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
  if (li >= plan.n_long || row_failed[li]) return;
  const int u = plan.rows[li];
  float *xrow = X + (size_t)u * f;
  for (int i = lane; i < f; i += 64) xs[i] = xrow[i];
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  float gs = 0.f;
  for (int sg = plan.row_seg[li]; sg < plan.row_seg[li + 1]; ++sg) {
    const float *in = partials + (size_t)sg * kSubPartial + lane;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] += in[e * 64];
    gs += in[16 * 64];
  }
  wave_lds_fence();
  if (!solve_block<K>(acc, gs, G, xs, Hs, dl, f, s0, kb, reg, lane)) {
    if (lane == 0) {
      row_failed[li] = 1;
      atomicMin(failed_row, (unsigned long long)u);
    }
    return;
  }
  if (lane < kb) xrow[s0 + lane] = xs[s0 + lane];
  if (lane < K) delta[(size_t)li * 32 + lane] = dl[lane];
}

// one wavefront per segment: p_j += delta . y_j[S]
__global__ __launch_bounds__(256) void subspace_long_update_kernel(const LongPlanDev plan, const int32_t *__restrict__ indices,
                                                                   const float *__restrict__ Y, float *pred, int f, int s0, int kb,
                                                                   const int *__restrict__ row_failed, const float *__restrict__ delta) {
  __shared__ float dl_all[4][32];
  const int lane = threadIdx.x & 63;
  float *dl = dl_all[threadIdx.x >> 6];
  const int sg = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
  if (sg >= plan.n_seg) return;
  const int li = plan.seg_row[sg];
  if (row_failed[li]) return;
  if (lane < 32) dl[lane] = lane < kb ? delta[(size_t)li * 32 + lane] : 0.f;
  wave_lds_fence();
  predict_range<false>(indices, Y, pred, plan.seg_begin[sg], plan.seg_end[sg], f, s0, kb, dl, lane);
}

template <int K>
static void subspace_launch(const imp_csr *C, float *X, const float *G, const float *Y, float *pred, int f, float reg, int block,
                            int sweeps, unsigned long long *g_failed) {
  const LongPlanDev plan = C->plan_chol.dev(C->order.data());
  if (plan.n_seg > 0) {
    // [n_seg] partials, [n_long][32] deltas, [n_long] failure flags of the rows
    const size_t need = (size_t)plan.n_seg * kSubPartial + (size_t)plan.n_long * 33;
    float *partials = ctx().subspace_ws.reserve(need), *delta = partials + (size_t)plan.n_seg * kSubPartial;
    int *row_failed = reinterpret_cast<int *>(delta + (size_t)plan.n_long * 32);
    IMP_CHECK_HIP(hipMemsetAsync(row_failed, 0, (size_t)plan.n_long * sizeof(int), stream()));
    const int seg_grid = (plan.n_seg + 3) / 4, row_grid = (plan.n_long + 3) / 4;
    IMP_PROF("als_subspace_long_rows");
    subspace_long_predict_kernel<<<seg_grid, 256, 0, stream()>>>(plan, C->indices.data(), X, Y, pred, f);
    for (int sw = 0; sw < sweeps; ++sw)
      for (int s0 = 0; s0 < f; s0 += block) {
        const int kb = std::min(block, f - s0);
        subspace_long_partial_kernel<<<seg_grid, 256, 0, stream()>>>(plan, C->indices.data(), C->data.data(), Y, pred, f, s0, kb,
                                                                      row_failed, partials);
        subspace_long_solve_kernel<K><<<row_grid, 256, 0, stream()>>>(plan, X, G, partials, f, s0, kb, reg, row_failed, delta, g_failed);
        subspace_long_update_kernel<<<seg_grid, 256, 0, stream()>>>(plan, C->indices.data(), Y, pred, f, s0, kb, row_failed, delta);
      }
    IMP_CHECK_HIP(hipGetLastError());
  }
  const int n_wave = C->nonempty() - plan.n_long;
  if (n_wave > 0) {
    IMP_PROF("als_subspace_wave_rows");
    const int grid = std::min((n_wave + 3) / 4, ctx().num_cus * 16);
    subspace_wave_kernel<K><<<grid, 256, 0, stream()>>>(C->order.data(), plan.n_long, n_wave, C->indptr.data(), C->indices.data(),
                                                        C->data.data(), X, Y, G, pred, f, reg, block, sweeps, g_failed);
    IMP_CHECK_HIP(hipGetLastError());
  }
}

// One block of rows (an imp_csr without parts).  Returns -1, or the smallest failing row.  Arguments are checked by the caller.
int64_t least_squares_subspace(const imp_csr *C, imp_matrix *X, const imp_matrix *YtY, const imp_matrix *Y, double reg, int block_size,
                               int sweeps) {
  const int f = (int)X->cols;
  float *const x = X->mut_rows<float>(0, (size_t)C->rows);  // the rows this call solves
  unsigned long long *g_failed = reset_fail_word();
  if (C->nonempty() > 0) {
    float *pred = ctx().subspace_pred.reserve((size_t)C->nnz);
    if (block_size <= 8) subspace_launch<8>(C, x, YtY->f32(), Y->f32(), pred, f, (float)reg, block_size, sweeps, g_failed);
    else if (block_size <= 16) subspace_launch<16>(C, x, YtY->f32(), Y->f32(), pred, f, (float)reg, block_size, sweeps, g_failed);
    else subspace_launch<32>(C, x, YtY->f32(), Y->f32(), pred, f, (float)reg, block_size, sweeps, g_failed);
  }
  zero_rows(C->order.data(), C->first_empty(), C->n_empty(), x, f);
  return read_fail_word(g_failed);
}

}  // namespace imp
