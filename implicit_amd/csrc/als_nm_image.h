// The LDS image of a row's explicit normal matrix (als_cg_nm.hip has the design) and what works on a COMPLETE image: the CG
// (nm_cg) and the finish items of the rows that were built in more than one segment (nm_finish_items).  Shared by the
// normal-matrix kernels and by the chain of the three 512-thread classes (als_cg_qf.hip), which carries the finish items at
// its head.
#ifndef IMPLICIT_AMD_CSRC_ALS_NM_IMAGE_H_
#define IMPLICIT_AMD_CSRC_ALS_NM_IMAGE_H_

#include "als_qtile.h"
#include "common.h"
#include "wave_ops.h"

namespace imp {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

template <int F> struct NmShape;
template <> struct NmShape<128> {
  static constexpr int M = 32, KG = 2, NACC = 16;
  using acc_t = f32x16;
  __device__ static __forceinline__ acc_t mfma(half8 a, half8 b, acc_t c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
  // C/D layout of the 32 x 32 tile: column = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
  __device__ static __forceinline__ int row(int lane, int e) { return (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5); }
  __device__ static __forceinline__ int col(int lane) { return lane & 31; }
};
template <> struct NmShape<64> {
  static constexpr int M = 16, KG = 4, NACC = 4;
  using acc_t = f32x4v;
  __device__ static __forceinline__ acc_t mfma(half8 a, half8 b, acc_t c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
  // 16 x 16 tile: column = lane & 15, row = 4 (lane >> 4) + e
  __device__ static __forceinline__ int row(int lane, int e) { return 4 * (lane >> 4) + e; }
  __device__ static __forceinline__ int col(int lane) { return lane & 15; }
};

template <int F> struct NmLayout {
  static constexpr int M = F / 4;              // rows of a tile
  static constexpr int TS = M + 1;             // row stride inside a tile: rows m and columns n both walk all LDS banks
  static constexpr int IMG = 16 * M * TS;      // floats of the image: 16 tiles (I, J), tile (I, J)[m][n] = A[4m+I][4n+J]
  static constexpr int KCH = 8 * NmShape<F>::KG;  // nonzeros per step (one wavefront's gathers)
  static constexpr int ROUND = 4 * KCH;        // nonzeros per round: one step from each of the four wavefronts
  static constexpr int kTiles = 10;            // (I, J), I >= J
  static constexpr int kSlots = 3;             // tiles per wavefront: 3, 3, 2, 2
  // operand exchange: [step][kind: uh ul yh yl][block][lane] quads of 16 bytes
  static constexpr int QUAD = 64 * 4;          // floats of one operand quad (one b128 per lane)
  static constexpr int OPS = 4 * 16 * QUAD;    // floats of the exchange buffer (64 KB); the image re-uses the space afterwards
  static constexpr int NP = 256 / F;           // thread groups sharing a matrix row in the CG phase
  static constexpr int kVec = IMG > OPS ? IMG : OPS;  // offset of the vectors behind the image / exchange buffer
  static constexpr size_t lds_floats = (size_t)kVec + 2 * F + NP * F + 64 + 4 * F;  // image / operands | b | p | partial products | reduction slots | b per wavefront
  __host__ __device__ static constexpr int at(int I, int J, int m, int n) { return ((I * 4 + J) * M + m) * TS + n; }
};

// ---- CG on the LDS image (als.cu:45-109 with A_u p from the explicit matrix) ----------------------------------------------------
// Vectors live in image order: position r = I M + m is factor 4m + I.  Thread (r = tid % F, grp = tid / F) forms the products of
// row r with the column blocks J of its group: lanes walk m, i.e. consecutive tile rows of stride M + 1 -- conflict-free.
// Written for 256 threads.  BLOCK > 256 (the finish items of the 512-thread chain): the wavefronts from the fifth on take every
// workgroup barrier and nothing else -- they read the same scalars as the others, so every return is uniform over the workgroup.
template <int F, typename T, int BLOCK = 256>
__device__ __forceinline__ bool nm_cg(const float *img, const float *bvec, float *pv, float *parts, float *red, T *xrow, int cg_steps, int tid) {
  using L = NmLayout<F>;
  constexpr int M = L::M, NP = L::NP, JPG = 4 / NP;
  static_assert(BLOCK >= 256 && BLOCK % 64 == 0, "256 working threads, whole wavefronts beside them");
  const bool on = BLOCK == 256 || tid < 256;  // wave-uniform
  const int r = tid % F, grp = tid / F, lane = tid & 63, wave = tid >> 6;
  const int I = r / M, m = r % M;
  int slot = 0;
  auto matvec = [&]() {
    if (on) {
      float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int jj = 0; jj < JPG; ++jj) {
        const int J = grp * JPG + jj;
        const float *row = img + L::at(I, J, m, 0);
#pragma unroll
        for (int n = 0; n < M; n += 4) {
          const float4 p4 = *reinterpret_cast<const float4 *>(pv + J * M + n);
          s[0] = fmaf(row[n], p4.x, s[0]), s[1] = fmaf(row[n + 1], p4.y, s[1]);
          s[2] = fmaf(row[n + 2], p4.z, s[2]), s[3] = fmaf(row[n + 3], p4.w, s[3]);
        }
      }
      parts[grp * F + r] = (s[0] + s[1]) + (s[2] + s[3]);
    }
    __syncthreads();
    float q = parts[r];
#pragma unroll
    for (int gq = 1; gq < NP; ++gq) q += parts[gq * F + r];
    return q;
  };
  auto block_sum = [&](float v) {  // over the F positions (the threads of group 0 contribute)
    if (on) {
      v = wave_allsum(grp == 0 ? v : 0.f);
      if (lane == 0) red[4 * slot + wave] = v;
    }
    __syncthreads();
    const float s = (red[4 * slot] + red[4 * slot + 1]) + (red[4 * slot + 2] + red[4 * slot + 3]);
    slot = (slot + 1) & 7;
    return s;
  };
  // Operands beyond the fp16 range leave infinities in the image; whatever they touch stops being finite.  The squared norms
  // below see every component of every residual and of every A p (through p.Ap) -- one non-finite value in them and the row is
  // NOT stored: the caller lists it for the fp32 fix-up kernel.  (A row whose inputs are not finite to begin with takes the same
  // way and gets the reference's own non-finite answer there.)
  auto finite = [](float v) { return fabsf(v) <= 3.0e38f; };
  float x = on ? load1(xrow + 4 * m + I) : 0.f;
  if (grp == 0) pv[r] = x;
  __syncthreads();
  float res = bvec[r] - matvec();
  float p = res;
  float rsold = block_sum(res * res);
  if (!finite(rsold)) return true;
  if (rsold < 1e-20f) return false;
  for (int it = 0; it < cg_steps; ++it) {
    if (grp == 0) pv[r] = p;
    __syncthreads();
    const float Ap = matvec();
    const float pAp = block_sum(p * Ap);
    const float alpha = rsold / pAp;
    x = fmaf(alpha, p, x);
    res = fmaf(-alpha, Ap, res);
    const float rsnew = block_sum(res * res);
    if (!finite(pAp) || !finite(rsnew) || !finite(alpha)) return true;
    if (rsnew < 1e-20f) break;
    p = fmaf(rsnew / rsold, p, res);
    rsold = rsnew;
  }
  if (grp == 0) store1(xrow + 4 * m + I, x);
  return false;
}

// ---- finish items: the rows of more than one segment, one workgroup per row at a time ------------------------------------------
// What als_cg_nm_reduce_kernel + als_cg_nm_finish_kernel do in two launches, as the head of a launch that follows the
// normal-matrix kernel anyway: workgroup b takes the rows li = b, b + gridDim.x, ... of the first n_multi of the plan.
struct NmFinishArgs {
  int n_multi = 0;               // 0: nothing to finish
  const int32_t *rows = nullptr;     // LongPlanDev::rows
  const int32_t *row_seg = nullptr;  // LongPlanDev::row_seg
  const float *gram_img = nullptr, *partial = nullptr;
  int *ctl = nullptr;            // [2]: rows listed for the fix-up
  unsigned *fix_rows = nullptr;
};

// The image of a row into the LDS: the gramian image plus the partial images of segments s0 .. s1 - 1 ADDED ONE AFTER THE OTHER
// in segment order, the b parts (behind the image in a partial, and behind it in the LDS at f = 128) from zero -- the order of
// als_cg_nm_reduce_kernel, so the sums carry the same bits.  Nothing is written back to the workspace: the stand-alone reduce
// kernel leaves a row's sum in the partial of its first segment, this route leaves the partials as the normal-matrix kernel
// wrote them -- nobody may rely on partial[first segment] holding the sum after a half sweep.  A thread owns whole
// 16-byte pieces and keeps kInFlight loads of them in the air: kSegBatch segments of two pieces, or -- rows of few segments, most
// of them -- two segments of eight pieces.  Loads past a row's last segment or the last piece re-read the last one and are dropped.
constexpr int kNmSegBatch = 8;
template <int F, int BLOCK, int P, int S>
__device__ __forceinline__ void nm_sum_partials_shape(const float4 *__restrict__ gram4, const float4 *__restrict__ part4, int s0, int s1,
                                                      float *img, float *bvec, int tid) {
  using L = NmLayout<F>;
  constexpr int NIMG = L::IMG / 4, TOTAL = NIMG + F / 4;
  constexpr size_t stride = (size_t)(L::IMG + F) / 4;  // float4 pieces per partial
  for (int e0 = tid; e0 < TOTAL; e0 += BLOCK * P) {
    float4 sum[P];
    int e[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      e[p] = min(e0 + p * BLOCK, TOTAL - 1);
      sum[p] = e[p] < NIMG ? gram4[e[p]] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int s = s0; s < s1; s += S) {
      float4 v[P][S];
#pragma unroll
      for (int q = 0; q < S; ++q)
#pragma unroll
        for (int p = 0; p < P; ++p) v[p][q] = part4[(size_t)min(s + q, s1 - 1) * stride + e[p]];
#pragma unroll
      for (int q = 0; q < S; ++q) {
        if (s + q < s1) {  // uniform
#pragma unroll
          for (int p = 0; p < P; ++p) sum[p].x += v[p][q].x, sum[p].y += v[p][q].y, sum[p].z += v[p][q].z, sum[p].w += v[p][q].w;
        }
      }
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int ep = e0 + p * BLOCK;
      if (ep < NIMG) reinterpret_cast<float4 *>(img)[ep] = sum[p];
      else if (ep < TOTAL) reinterpret_cast<float4 *>(bvec)[ep - NIMG] = sum[p];
    }
  }
}

// smem: NmLayout<F>::lds_floats floats.  Returns behind a workgroup barrier (the caller may re-use the allocation) when the
// workgroup had an item, at once otherwise; uniform over the workgroup either way.
template <int F, typename T, int BLOCK>
__device__ __forceinline__ void nm_finish_items(const NmFinishArgs &a, T *__restrict__ X, int cg_steps, float *smem) {
  using L = NmLayout<F>;
  static_assert(L::IMG % 4 == 0 && F % 4 == 0, "the image and b are moved in 16-byte pieces");
  float *img = smem, *bvec = img + L::kVec, *pv = bvec + F, *parts = pv + F, *red = parts + L::NP * F;
  const int tid = threadIdx.x;
  const float4 *gram4 = reinterpret_cast<const float4 *>(a.gram_img), *part4 = reinterpret_cast<const float4 *>(a.partial);
  for (int li = blockIdx.x; li < a.n_multi; li += gridDim.x) {
    const int s0 = a.row_seg[li], s1 = a.row_seg[li + 1];
    if (s1 - s0 > 4) nm_sum_partials_shape<F, BLOCK, 2, kNmSegBatch>(gram4, part4, s0, s1, img, bvec, tid);
    else nm_sum_partials_shape<F, BLOCK, 8, 2>(gram4, part4, s0, s1, img, bvec, tid);
    __syncthreads();
    const bool bad = nm_cg<F, T, BLOCK>(img, bvec, pv, parts, red, X + (size_t)a.rows[li] * F, cg_steps, tid);
    if (bad && tid == 0) a.fix_rows[atomicAdd(a.ctl + 2, 1)] = (unsigned)a.rows[li];
    __syncthreads();  // the CG has read the image and b: the next item, or the caller, may overwrite them
  }
}

}  // namespace imp

#endif  // IMPLICIT_AMD_CSRC_ALS_NM_IMAGE_H_
