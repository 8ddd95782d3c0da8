// K4: top-k dot-product scorer behind recommend() / similar_items() / similar_users().
//
// Replaces KnnQuery::topk (implicit/gpu/knn.cu:77-265: cuBLAS GEMM + three Thrust passes + RAFT
// select_k).  Semantics follow the CPU oracle implicit/cpu/topk.pyx:15-67 + select.h:12-40:
//   scores = query . items^T (exact fp32), optional divide by item_norms, per-query (COO) and global
//   item filters set to -FLT_MAX, then the k best per row, written best-first.
// Output order (score desc, column desc) is the oracle's.  When more entries tie with the k-th score than
// there are places left, the retained set follows the reference heap's arrival-order rule exactly
// (closed form at "the tie rule" in topk_select.h), so ids are bit-identical to select.h even on all-zero / all-filtered rows.
//
// Stage 1  score_gemm_kernel : fp32 MFMA (v_mfma_f32_32x32x2_f32), LDS-staged K-tiles of both operands
//          with odd row stride (conflict-free fragment reads), norm divide fused in the epilogue.
// Stage 2  filters (tiny scatter kernels).
// Stage 3  select_kernel (topk_select.h) : one workgroup per query row, MSB-first 8-bit radix select on the 64-bit key
//          (ordered(score) << 32 | column) over the score bytes with early exit once the boundary bucket
//          is taken whole, exact tie resolution otherwise, a gather of the k winners and an in-LDS bitonic sort.
//
// This file: the scoring GEMMs, the filter and bitmap kernels and the host routes.  select_ops.h has the key, sort and radix
// primitives, topk_select.h every select kernel, topk_resident.h the fp16 two-term GEMM with resident queries.
#include <cfloat>
#include <type_traits>

#include "als_qtile.h"  // load4: fp32 / fp16 factor storage converted in registers
#include "common.h"
#include "select_ops.h"
#include "topk_resident.h"
#include "topk_select.h"

namespace imp {

constexpr int kBM = 64;   // queries per block tile
constexpr int kBN = 128;  // items per block tile
constexpr int kBK = 64;   // factors per K step
constexpr int kLd = kBK + 1;

// scores[q][i] = sum_k Q[q][k] * I[i][k]   (optionally / norms[i])
__global__ __launch_bounds__(256) void score_gemm_kernel(const float *__restrict__ Q, int nq, const float *__restrict__ I,
                                                         int ni, int f, const float *__restrict__ norms,
                                                         float *__restrict__ S) {
  __shared__ float Qs[kBM * kLd];
  __shared__ float Is[kBN * kLd];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = blockIdx.y * kBM, i0 = blockIdx.x * kBN;
  f32x16 acc[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;

  for (int k0 = 0; k0 < f; k0 += kBK) {
    // stage: consecutive threads walk the factor dimension -> coalesced global reads
    for (int e = tid; e < kBM * kBK; e += 256) {
      int r = e / kBK, c = e - r * kBK;
      int q = q0 + r, k = k0 + c;
      Qs[r * kLd + c] = (q < nq && k < f) ? Q[(size_t)q * f + k] : 0.f;
    }
    for (int e = tid; e < kBN * kBK; e += 256) {
      int r = e / kBK, c = e - r * kBK;
      int i = i0 + r, k = k0 + c;
      Is[r * kLd + c] = (i < ni && k < f) ? I[(size_t)i * f + k] : 0.f;
    }
    __syncthreads();
    // wave w: queries [0,64) x items [32w, 32w+32): two 32x32 tiles
    const int kh = lane >> 5, l31 = lane & 31;
#pragma unroll 8
    for (int kk = 0; kk < kBK; kk += 2) {
      float b = Is[(32 * wave + l31) * kLd + kk + kh];
      float a0 = Qs[l31 * kLd + kk + kh];
      float a1 = Qs[(32 + l31) * kLd + kk + kh];
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc[1], 0, 0, 0);
    }
    __syncthreads();
  }
  const int item = i0 + 32 * wave + (lane & 31);
  if (item < ni) {
    float inv_valid = norms ? norms[item] : 1.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        int q = q0 + 32 * t + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        if (q < nq) {
          float s = acc[t][e];
          if (norms) s = s / inv_valid;
          S[(size_t)q * ni + item] = s;
        }
      }
  }
}

__global__ void item_filter_kernel(float *__restrict__ S, int rows, int ni, const int32_t *__restrict__ items, int n_items) {
  size_t total = (size_t)rows * n_items;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    int col = items[i % n_items];
    size_t row = i / n_items;
    if (col >= 0 && col < ni) S[row * ni + col] = -FLT_MAX;
  }
}

__global__ void coo_filter_kernel(float *__restrict__ S, int start, int end, int ni, const int32_t *__restrict__ row,
                                  const int32_t *__restrict__ col, size_t nnz) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < nnz; i += (size_t)gridDim.x * blockDim.x) {
    int r = row[i], c = col[i];
    if (r >= start && r < end && c >= 0 && c < ni) S[(size_t)(r - start) * ni + c] = -FLT_MAX;
  }
}

// ---- fast path (f % 8 == 0): 128 x 128 block tile, 4 waves as 2 x 2, each wave 64 queries x 64 items = 2 x 2 MFMA tiles -----
// Split-bf16 form (f % 16 == 0; materialising path and fallback): v_mfma_f32_32x32x16_bf16 on three-way split operands, both
// operands staged per workgroup and 16-factor step by LDS-DMA (see the kernel).  fp16 form (f % 16 == 0; the emit path's two
// GEMMs, round 5): the same staging, two fp16 terms per value and three products (H2 at split8_f16).  Exact-fp32 form (v_mfma_f32_32x32x2_f32; f % 8 == 0 off the
// 16-grid, IMP_TOPK_FP32_MFMA=1): operands straight from global memory, no LDS, no barriers -- lane (r = l & 31, kh = l >> 5)
// loads ONE float4 = 4 consecutive factors [k0 + 4 kh, +4) of its query / item row per 8-factor block; MFMA step s of the
// block uses factor k0 + 4 kh + s for BOTH operands (the k index inside an MFMA is a free permutation), so one dwordx4 per
// operand tile feeds 4 MFMAs.  Epilogues: optional divide by the item norm, then the coalesced score write with the
// per-(query, 64-item = kTileItems) maximum for the pruned select (MODE 0), the compact threshold subset (1) or the emit test (2).
//
// MODE 0: scores written to S[q][item] + per-(query, 64-item) maxima          (materialising path)
// MODE 1: only every `block_stride`-th 128-item block is computed, into the compact S[q][128 b + ...] (threshold pre-pass)
// MODE 2: nothing is materialised: scores >= tau[q] that are not filtered (bitmaps) are appended to the query's candidate list
//         (EmitArgs, topk_select.h)
//
// TQ / TI: storage type of the query / item factors (float or __half).  fp16 factors are read as they are stored and
// converted in registers (8-byte loads; the reference hands fp16 operands straight to the GEMM with fp32 accumulation,
// implicit/gpu/knn.cu:117-128) -- bit-identical to scoring an fp32 copy, without writing and re-reading one per call.
//
// BF3 (f % 16 == 0, the default): the product on the bf16 matrix cores with every operand value split into three bf16 terms
// in registers (hi + mid + lo = the fp32 value to 2^-24) and the six partial products down to 2^-16 relative weight accumulated
// in fp32, smallest first ("3xBF16"): measured error against fp64 BELOW that of an fp32 FMA chain (2.6e-8 vs 2e-7 relative at
// f = 128), 24 v_mfma_f32_32x32x16_bf16 per 16 factors of a 64 x 64 wave tile instead of 32 v_mfma_f32_32x32x2_f32 at twice
// the instruction time each -- the fp32 MFMA runs at the VECTOR rate, 1/16 of the bf16 rate.  The splits (11 vector
// instructions per pair of values) run on the vector pipe beside the matrix pipe.  A and B fragments share the
// (lane >> 5, element) -> k assignment, which is all the contraction needs; C/D layout is that of the fp32 form.
typedef __bf16 tk_bf16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ void split8_bf16(const float4 &v0, const float4 &v1, tk_bf16x8 &h, tk_bf16x8 &m, tk_bf16x8 &l) {
  const float x[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const __bf16 hi = (__bf16)x[e];
    const float r1 = x[e] - (float)hi;
    const __bf16 mid = (__bf16)r1;
    h[e] = hi, m[e] = mid, l[e] = (__bf16)(r1 - (float)mid);
  }
}

// Query rows split ahead of the GEMM (emit path) and stored in FRAGMENT order: for every tile of 32 query rows, step of 16
// factors and term (hi, mid, lo -- the same bits split8_bf16 produces) the 64 lanes' 8-element operands lie side by side, so
// a wavefront's operand load is ONE contiguous KB (8 whole cache lines) instead of 64 pieces of 16 bytes in 32 lines, and the
// 2 x n_item_blocks workgroups that read a query block no longer repeat the split (1000 x 128 values once against 2285 times
// at configs[2]).  Rows are padded to whole 128-row query blocks with zeros.  `TQ = split_bf16` selects it in score_gemm_direct_kernel
// (Q then points at the first tile of the launch).  IMP_TOPK_NO_QSPLIT=1: split in the GEMM as for the items (A/B).
struct split_bf16 {
  __bf16 v;
};
template <typename T>
__global__ void split_query_rows_kernel(const T *__restrict__ Q, __bf16 *__restrict__ out, size_t rows, size_t rows_pad, int f) {
  const size_t n = rows_pad * (size_t)f;
  const int steps16 = f / 16;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t q = i / f;
    const int c = (int)(i - q * f);
    const float x = q < rows ? (float)Q[i] : 0.f;
    const __bf16 hi = (__bf16)x;
    const float r1 = x - (float)hi;
    const __bf16 mid = (__bf16)r1;
    const int lane = (int)(q & 31) + 32 * ((c >> 3) & 1);
    __bf16 *o = out + ((((q >> 5) * steps16 + (c >> 4)) * 3) * 64 + lane) * 8 + (c & 7);
    o[0] = hi, o[64 * 8] = mid, o[2 * 64 * 8] = (__bf16)(r1 - (float)mid);
  }
}

template <typename TQ> struct presplit {
  static constexpr int terms = 0;
};
template <> struct presplit<split_bf16> {
  static constexpr int terms = 3;
};

// four consecutive factors as they are stored, and their fp32 values
template <typename T> struct raw4 {
  using type = float4;
};
template <> struct raw4<__half> {
  using type = uint2;
};
template <typename T> using raw4_t = typename raw4<T>::type;
__device__ __forceinline__ float4 load_raw4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ uint2 load_raw4(const __half *p) { return *reinterpret_cast<const uint2 *>(p); }
__device__ __forceinline__ float4 widen4(const float4 &v) { return v; }
__device__ __forceinline__ float4 widen4(const uint2 &raw) {
  const float2 a = __half22float2(*reinterpret_cast<const __half2 *>(&raw.x));
  const float2 b = __half22float2(*reinterpret_cast<const __half2 *>(&raw.y));
  return make_float4(a.x, a.y, b.x, b.y);
}

#ifndef IMP_TOPK_MIN_WAVES
#define IMP_TOPK_MIN_WAVES 3  // waves per SIMD the register allocation leaves room for (split-bf16 emit GEMM at C3: 2 waves 0.83 ms, 3: 0.73, 4: 0.80)
#endif
template <int MODE, typename TQ = float, typename TI = float, bool BF3 = false>
__global__ __launch_bounds__(256, IMP_TOPK_MIN_WAVES) void score_gemm_direct_kernel(const TQ *__restrict__ Q, int nq, const TI *__restrict__ I,
                                                                int ni, int f, const float *__restrict__ norms,
                                                                float *__restrict__ S, float *__restrict__ tile_max,
                                                                int n_tiles, int block_stride, EmitArgs emit) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, kh = lane >> 5;
  const int q_base = blockIdx.y * 128 + 64 * (wave >> 1);
  const int i_base = (MODE == 1 ? blockIdx.x * block_stride : blockIdx.x) * 128 + 64 * (wave & 1);
  constexpr bool QS = presplit<TQ>::terms > 0;  // query rows already split, in fragment order: 3 bf16 or 2 fp16 terms per value
  constexpr int NT = QS ? presplit<TQ>::terms : 3;
  static_assert(!QS || BF3, "split query rows feed the matrix-core forms only");
  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

  if constexpr (BF3) {
    // 16 factors per step, both operands through LDS, staged ONCE per workgroup and step by LDS-DMA (no staging registers):
    // a wavefront load of lane (r, kh)'s own 16 bytes of its row touches 32 cache lines for 1 KB, and with every wave loading
    // its own operands each tile crossed L2 -> L1 twice; the texture addresser and the L2 port, not the matrix pipe, set the
    // pace (emit GEMM at configs[2]: 0.72 ms that way; 0.56 with the queries in fragment order; 0.52 with wave-private LDS
    // staging of the items; knock-outs: MFMAs 0.17 ms, loads 0.17, splits 0.07, epilogue 0.06-0.27).
    //  * factor ROWS (items; queries when they are not pre-split): 1 KB per DMA instruction = whole 64- / 32-byte row pieces
    //    (16 rows fp32, 32 rows fp16), the 16-byte chunks of a row XOR-swizzled -- on the SOURCE side, the DMA destination is
    //    lane-linear -- so that the 32 rows of a fragment read spread over all banks;
    //  * pre-split queries: 12 (8) fragment pieces of 1 KB (4 tiles x 3 bf16 / 2 fp16 terms), lane-linear as stored.
    // The 8 (4) + 12 (8) instructions of a step are dealt to the four waves; double buffer, one barrier per step: a wave requests
    // step s + 1 after the barrier of step s, which every wave reaches only with its fragment reads of step s - 1 consumed.
    constexpr int CHI = (int)sizeof(TI), CHQ = QS ? 4 : (int)sizeof(TQ);  // 16-byte chunks per row and step: 4 (fp32), 2 (fp16)
    constexpr int Q_BYTES = QS ? 4 * NT * 1024 : CHQ * 2048, I_BYTES = CHI * 2048;
    __shared__ __attribute__((aligned(1024))) unsigned char stage[2][Q_BYTES + I_BYTES];
    const int i_block = i_base - 64 * (wave & 1), q_block = q_base - 64 * (wave >> 1);
    // DMA sources of this wave (rows are clamped: what the extra rows produce is discarded)
    constexpr int NI_W = 2 * CHI / 4, NQ_W = QS ? NT : 2 * CHQ / 4;  // instructions per wave and step
    const TI *isrc[NI_W];
    const void *qsrc[NQ_W];
#pragma unroll
    for (int i = 0; i < NI_W; ++i) {
      const int j = wave + 4 * i, rho = lane / CHI, pos = lane % CHI, sw = (rho / (8 / CHI)) & (CHI - 1);
      isrc[i] = I + (size_t)min(i_block + j * (64 / CHI) + rho, ni - 1) * f + (pos ^ sw) * (16 / (int)sizeof(TI));
    }
#pragma unroll
    for (int i = 0; i < NQ_W; ++i) {
      if constexpr (QS) {
        const int idx = wave * NT + i, tile = idx / NT, plane = idx % NT;
        qsrc[i] = reinterpret_cast<const uint16_t *>(Q) + (((size_t)(q_block / 32 + tile) * (f / 16)) * NT + plane) * 512 + lane * 8;
      } else {
        const int j = wave + 4 * i, rho = lane / CHQ, pos = lane % CHQ, sw = (rho / (8 / CHQ)) & (CHQ - 1);
        qsrc[i] = Q + (size_t)min(q_block + j * (64 / CHQ) + rho, nq - 1) * f + (pos ^ sw) * (16 / (int)sizeof(TQ));
      }
    }
    auto dma = [&](int buf, int s16) {
#pragma unroll
      for (int i = 0; i < NQ_W; ++i) {
        const unsigned char *src = reinterpret_cast<const unsigned char *>(qsrc[i]) + (QS ? (size_t)s16 * NT * 1024 : (size_t)s16 * 16 * sizeof(TQ));
        const int slot = QS ? wave * NT + i : wave + 4 * i;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                         (__attribute__((address_space(3))) void *)&stage[buf][slot * 1024], 16, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < NI_W; ++i)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(isrc[i] + 16 * s16),
                                         (__attribute__((address_space(3))) void *)&stage[buf][Q_BYTES + (wave + 4 * i) * 1024], 16, 0, 0);
    };
    // fragment offsets of lane (r, kh): row R of a 128-row region -> piece R / rows-per-piece, swizzled chunk
    auto row_offset = [&](int R, int CH) {
      const int rpi = 64 / CH, j = R / rpi, rh = R % rpi, sw = (rh / (8 / CH)) & (CH - 1), c0 = CH == 4 ? 2 * kh : kh;
      return j * 1024 + (rh * CH + (c0 ^ sw)) * 16;
    };
    int q_off[2], i_off[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      i_off[t] = Q_BYTES + row_offset(64 * (wave & 1) + 32 * t + r, CHI);
      q_off[t] = QS ? ((2 * (wave >> 1) + t) * NT * 64 + lane) * 16 : row_offset(64 * (wave >> 1) + 32 * t + r, CHQ);
    }
    auto read_rows = [&](const unsigned char *base, int off, int CH, float4 &v0, float4 &v1) {
      if (CH == 4) {
        v0 = *reinterpret_cast<const float4 *>(base + off);
        v1 = *reinterpret_cast<const float4 *>(base + (off ^ 16));
      } else {
        const uint4 raw = *reinterpret_cast<const uint4 *>(base + off);
        v0 = widen4(uint2{raw.x, raw.y}), v1 = widen4(uint2{raw.z, raw.w});
      }
    };
    auto multiply16 = [&](int buf) {
      const unsigned char *base = &stage[buf][0];
      tk_bf16x8 ah[2], am[2], al[2], bh[2], bm[2], bl[2];
      float4 ra[2][2], rb[2][2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if constexpr (QS) {
          ah[t] = *reinterpret_cast<const tk_bf16x8 *>(base + q_off[t]);
          am[t] = *reinterpret_cast<const tk_bf16x8 *>(base + q_off[t] + 1024);
          al[t] = *reinterpret_cast<const tk_bf16x8 *>(base + q_off[t] + 2048);
        } else if constexpr (!QS) {
          read_rows(base, q_off[t], CHQ, ra[t][0], ra[t][1]);
        }
        read_rows(base, i_off[t], CHI, rb[t][0], rb[t][1]);
      }
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if constexpr (!QS) split8_bf16(ra[t][0], ra[t][1], ah[t], am[t], al[t]);
        split8_bf16(rb[t][0], rb[t][1], bh[t], bm[t], bl[t]);
      }
      return [=](auto &accr) {
#pragma unroll
        for (int tq = 0; tq < 2; ++tq)
#pragma unroll
          for (int ti = 0; ti < 2; ++ti) {
            f32x16 c = accr[tq][ti];
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[tq], bh[ti], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[tq], bl[ti], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[tq], bm[ti], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[tq], bh[ti], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[tq], bm[ti], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[tq], bh[ti], c, 0, 0, 0);
            accr[tq][ti] = c;
          }
      };
    };
    const int steps16 = f / 16;
    dma(0, 0);
    for (int s16 = 0; s16 < steps16; ++s16) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's pieces of step s16 have landed ...
      __syncthreads();                                   // ... and so have everybody else's
      auto products = multiply16(s16 & 1);             // fragments out of LDS, splits
      if (s16 + 1 < steps16) dma((s16 + 1) & 1, s16 + 1);
      products(acc);
    }
  } else {
  // 8 factors per step; the operands of step s + 1 are requested before the 16 MFMAs of step s (two register sets), so
  // the L2 round trip of a step hides under the matrix work of the previous one
  const TQ *qp[2];
  const TI *ip[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    qp[t] = Q + (size_t)min(q_base + 32 * t + r, nq - 1) * f + 4 * kh;  // clamped rows: results are discarded
    ip[t] = I + (size_t)min(i_base + 32 * t + r, ni - 1) * f + 4 * kh;
  }
  raw4_t<TQ> a0[2], a1[2];
  raw4_t<TI> b0[2], b1[2];
  auto fetch = [&](raw4_t<TQ> (&a)[2], raw4_t<TI> (&b)[2], int k0) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      a[t] = load_raw4(qp[t] + k0);
      b[t] = load_raw4(ip[t] + k0);
    }
  };
  auto multiply = [&](const raw4_t<TQ> (&ar)[2], const raw4_t<TI> (&br)[2]) {
    const float4 a[2] = {widen4(ar[0]), widen4(ar[1])}, b[2] = {widen4(br[0]), widen4(br[1])};
#pragma unroll
    for (int tq = 0; tq < 2; ++tq)
#pragma unroll
      for (int ti = 0; ti < 2; ++ti) {
        acc[tq][ti] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tq].x, b[ti].x, acc[tq][ti], 0, 0, 0);
        acc[tq][ti] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tq].y, b[ti].y, acc[tq][ti], 0, 0, 0);
        acc[tq][ti] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tq].z, b[ti].z, acc[tq][ti], 0, 0, 0);
        acc[tq][ti] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tq].w, b[ti].w, acc[tq][ti], 0, 0, 0);
      }
  };
  const int steps = f / 8;
  fetch(a0, b0, 0);
  int s = 0;
  for (; s + 2 <= steps; s += 2) {
    fetch(a1, b1, 8 * (s + 1));
    multiply(a0, b0);
    fetch(a0, b0, 8 * min(s + 2, steps - 1));  // past the end: re-reads the last step, unused
    multiply(a1, b1);
  }
  if (s < steps) multiply(a0, b0);
  }
  // C/D layout: column (item) = lane & 31, row (query) = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
  float nrm[2];
#pragma unroll
  for (int ti = 0; ti < 2; ++ti) {
    int item = i_base + 32 * ti + r;
    nrm[ti] = (norms && item < ni) ? norms[item] : 1.f;
  }
  // cosine scores: ONE wave-uniform branch around the 64 divisions.  Written per element ("if (norms) sc = sc / nrm") the
  // compiler turned the test into a select and every lane ran 64 IEEE division sequences (~700 vector instructions, more
  // than half of the main loop's count at f = 128) in recommend() calls, which have no norms at all.
  if (norms) {
#pragma unroll
    for (int tq = 0; tq < 2; ++tq)
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[tq][ti][e] = acc[tq][ti][e] / nrm[ti];
  }
  if constexpr (MODE == 1) {
    // compact layout: block b of the subset occupies columns [128 b, 128 b + 128); items past the end score -FLT_MAX
    const int sub_cols = gridDim.x * 128;
    const int c_base = blockIdx.x * 128 + 64 * (wave & 1);
#pragma unroll
    for (int tq = 0; tq < 2; ++tq)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int q = q_base + 32 * tq + (e & 3) + 8 * (e >> 2) + 4 * kh;
        if (q < nq) {
#pragma unroll
          for (int ti = 0; ti < 2; ++ti) {
            float sc = acc[tq][ti][e];
            S[(size_t)q * sub_cols + c_base + 32 * ti + r] = (i_base + 32 * ti + r < ni) ? sc : -FLT_MAX;
          }
        }
      }
    return;
  }
  if constexpr (MODE == 2) {
    // emission is rare (a few hundred scores per query row out of all items).  The thresholds of four consecutive query rows
    // come in one 16-byte load (the tau buffer is padded to whole 128-row blocks); a score is first compared with the
    // threshold as a float -- one instruction, true for every score the exact test accepts (and for a NaN) -- and only the
    // few that pass take the exact test on the ordered keys, the filter look-ups and the append.
#pragma unroll
    for (int tq = 0; tq < 2; ++tq)
#pragma unroll
      for (int eg = 0; eg < 4; ++eg) {
        const int q0 = q_base + 32 * tq + 8 * eg + 4 * kh;
        const uint4 t4 = *reinterpret_cast<const uint4 *>(emit.tau + q0);
        const uint32_t tk[4] = {t4.x, t4.y, t4.z, t4.w};
        // eight scores per lane against four thresholds, folded into one wave-wide test: most groups have no survivor
        bool any = false;
#pragma unroll
        for (int el = 0; el < 4; ++el) {
          const float tf = unordered(tk[el]);
          any |= !(acc[tq][0][4 * eg + el] < tf) | !(acc[tq][1][4 * eg + el] < tf);
        }
        if (__builtin_amdgcn_ballot_w64(any) == 0) continue;
#pragma unroll
        for (int el = 0; el < 4; ++el) {
          const int e = 4 * eg + el, q = q0 + el;
          const uint32_t t = tk[el];
          const float tf = unordered(t);
#pragma unroll
          for (int ti = 0; ti < 2; ++ti) {
            float sc = acc[tq][ti][e];
            if (!(sc < tf)) {
              if (!(sc == sc)) sc = INFINITY;  // (a NaN operand: select_candidates sends the row to the materialising path)
              const int item = i_base + 32 * ti + r;
              if (q < nq && item < ni && ordered(sc) >= t) {
                const uint32_t bit = 1u << (item & 31);
                bool filtered = emit.item_bits && (emit.item_bits[item >> 5] & bit);
                if (!filtered && emit.row_bits) filtered = emit.row_bits[(size_t)q * emit.words + (item >> 5)] & bit;
                if (!filtered) {
                  const unsigned int slot = atomicAdd(&emit.count[q], 1u);
                  if (slot < (unsigned)emit.cap) emit.cand[(size_t)q * emit.cap + slot] = make_key(sc, item);
                }
              }
            }
          }
        }
      }
    return;
  }
  const int tile = i_base / kTileItems;
  if (q_base + 64 <= nq && i_base + 64 <= ni) {
    // interior tile (wave-uniform): no per-element guards, so the 64 stores of a lane are queued back to back
#pragma unroll
    for (int tq = 0; tq < 2; ++tq)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int q = q_base + 32 * tq + (e & 3) + 8 * (e >> 2) + 4 * kh;
        float sc0 = acc[tq][0][e], sc1 = acc[tq][1][e];
        float *row = S + (size_t)q * ni + i_base + r;
        row[0] = sc0;
        row[32] = sc1;
        float m = fmaxf(sc0, sc1);
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
        if (r == 0) tile_max[(size_t)q * n_tiles + tile] = m;
      }
    return;
  }
#pragma unroll
  for (int tq = 0; tq < 2; ++tq)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int q = q_base + 32 * tq + (e & 3) + 8 * (e >> 2) + 4 * kh;
      float m = -FLT_MAX;
#pragma unroll
      for (int ti = 0; ti < 2; ++ti) {
        const int item = i_base + 32 * ti + r;
        float sc = acc[tq][ti][e];
        if (item < ni) {
          if (q < nq) S[(size_t)q * ni + item] = sc;
          m = fmaxf(m, sc);
        }
      }
      // maximum over the 32 lanes that hold this query row (same lane >> 5)
#pragma unroll
      for (int off = 16; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
      if (r == 0 && q < nq && tile < n_tiles) tile_max[(size_t)q * n_tiles + tile] = m;
    }
}

// After the filter scatters: recompute the maximum of every 64-item tile a filter touched (one thread per filter entry;
// several entries of one tile write the same value).  Keeps tau = the k-th largest tile maximum a valid AND tight lower
// bound without any slack for filtered entries.
__device__ __forceinline__ void refresh_tile_max(const float *__restrict__ S, float *__restrict__ tile_max, size_t row, int col,
                                                 int ni, int n_tiles) {
  const int tile = col / kTileItems;
  const int c0 = tile * kTileItems, c1 = min(ni, c0 + kTileItems);
  float m = -FLT_MAX;
  for (int c = c0; c < c1; ++c) m = fmaxf(m, S[row * ni + c]);
  tile_max[row * n_tiles + tile] = m;
}

__global__ void item_filter_refresh_kernel(const float *__restrict__ S, float *__restrict__ tile_max, int rows, int ni, int n_tiles,
                                           const int32_t *__restrict__ items, int n_items) {
  size_t total = (size_t)rows * n_items;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    int col = items[i % n_items];
    if (col >= 0 && col < ni) refresh_tile_max(S, tile_max, i / n_items, col, ni, n_tiles);
  }
}

__global__ void coo_filter_refresh_kernel(const float *__restrict__ S, float *__restrict__ tile_max, int start, int end, int ni,
                                          int n_tiles, const int32_t *__restrict__ row, const int32_t *__restrict__ col,
                                          size_t nnz) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < nnz; i += (size_t)gridDim.x * blockDim.x) {
    int r = row[i], c = col[i];
    if (r >= start && r < end && c >= 0 && c < ni) refresh_tile_max(S, tile_max, (size_t)(r - start), c, ni, n_tiles);
  }
}

// ---- emit path: top-k without the score matrix -----------------------------------------------------------------------
// The materialising path writes and re-reads batch x items scores (1.17 GB per 1000-query batch at 292 K items: the
// GEMM ran at the speed of that write, ~1 TB/s, not of the matrix pipe).  Here:
//   1. pre-pass: the scores of every kSubStride-th 128-item block (3 % of the items) go to a small buffer, filters are
//      applied to it, and tau[q] = its k-th largest entry -- a valid lower bound of the k-th best score over ALL items,
//      because those k entries are themselves unfiltered scores of the row;
//   2. the full GEMM (MODE 2) appends every unfiltered score >= tau[q] to the query's candidate list (about
//      kSubStride x k of them): filters are looked up in bitmaps, only for the scores that pass the threshold;
//   3. one workgroup per query sorts its candidates and writes the best k.  Overflowing lists, lists shorter than k and
//      an exact tie at the k-th score (the reference heap's arrival-order rule needs the whole row) raise `fallback`:
//      those queries are redone by the materialising path, 64 at a time.
// Scores are the same MFMA accumulations in both passes (same kernel body, same k order): bit-identical.
constexpr int kSubStride = 32;   // default / largest stride of the pre-pass subset (emit_stride() lowers it for large k)

__global__ void coo_bitmap_kernel(uint32_t *__restrict__ bits, int words, int start, int end, int ni, const int32_t *__restrict__ row,
                                  const int32_t *__restrict__ col, size_t nnz, float *__restrict__ S_sub, int sub_cols, int sub_stride) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < nnz; i += (size_t)gridDim.x * blockDim.x) {
    const int r = row[i], c = col[i];
    if (r < start || r >= end || c < 0 || c >= ni) continue;
    atomicOr(&bits[(size_t)(r - start) * words + (c >> 5)], 1u << (c & 31));
    const int blk = c >> 7;
    if (S_sub && blk % sub_stride == 0) S_sub[(size_t)(r - start) * sub_cols + (blk / sub_stride) * 128 + (c & 127)] = -FLT_MAX;
  }
}

// the words coo_bitmap_kernel touched, back to zero: a batch leaves its per-query bitmap as it found it, so the next batch needs no
// 36 MB memset (1000 queries x 292 385 items) -- this is 44 K stores, queued behind the batch where nobody waits for it
__global__ void coo_bitmap_clear_kernel(uint32_t *__restrict__ bits, int words, int start, int end, int ni, const int32_t *__restrict__ row,
                                        const int32_t *__restrict__ col, size_t nnz) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < nnz; i += (size_t)gridDim.x * blockDim.x) {
    const int r = row[i], c = col[i];
    if (r < start || r >= end || c < 0 || c >= ni) continue;
    bits[(size_t)(r - start) * words + (c >> 5)] = 0u;
  }
}

__global__ void item_bitmap_kernel(uint32_t *__restrict__ bits, int ni, const int32_t *__restrict__ items, int n_items,
                                   float *__restrict__ S_sub, int rows, int sub_cols, int sub_stride) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (size_t)n_items; i += (size_t)gridDim.x * blockDim.x) {
    const int c = items[i];
    if (c < 0 || c >= ni) continue;
    atomicOr(&bits[c >> 5], 1u << (c & 31));
    const int blk = c >> 7;
    if (blk % sub_stride == 0)
      for (int q = 0; q < rows; ++q) S_sub[(size_t)q * sub_cols + (blk / sub_stride) * 128 + (c & 127)] = -FLT_MAX;
  }
}

// fallback rows: query rows gathered into a compact matrix, filters replayed from the bitmaps onto the materialised scores
template <typename TQ>
__global__ void gather_query_rows_kernel(const TQ *__restrict__ Q, const int32_t *__restrict__ rows, int n, int f,
                                         float *__restrict__ out) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (size_t)n * f; i += (size_t)gridDim.x * blockDim.x)
    out[i] = load1(Q + (size_t)rows[i / f] * f + i % f);
}

__global__ void bitmap_filter_kernel(float *__restrict__ S, float *__restrict__ tile_max, int ni, int n_tiles,
                                     const int32_t *__restrict__ rows, int n, const uint32_t *__restrict__ row_bits,
                                     const uint32_t *__restrict__ item_bits, int words) {
  // one thread per (row, 64-item tile): clears the filtered scores of the tile and recomputes its maximum if any was hit
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (size_t)n * n_tiles; i += (size_t)gridDim.x * blockDim.x) {
    const int j = (int)(i / n_tiles), tile = (int)(i % n_tiles);
    uint32_t w0 = 0, w1 = 0;
    const int wi = 2 * tile;
    if (item_bits) {
      w0 |= item_bits[wi];
      if (wi + 1 < words) w1 |= item_bits[wi + 1];
    }
    if (row_bits) {
      const uint32_t *rb = row_bits + (size_t)rows[j] * words;
      w0 |= rb[wi];
      if (wi + 1 < words) w1 |= rb[wi + 1];
    }
    if (!(w0 | w1)) continue;
    float *srow = S + (size_t)j * ni;
    float m = -FLT_MAX;
    const int c0 = tile * kTileItems, c1 = min(ni, c0 + kTileItems);
    for (int c = c0; c < c1; ++c) {
      const uint32_t w = (c - c0) < 32 ? w0 : w1;
      if (w & (1u << (c & 31))) srow[c] = -FLT_MAX;
      m = fmaxf(m, srow[c]);
    }
    tile_max[(size_t)j * n_tiles + tile] = m;
  }
}

__global__ void scatter_topk_rows_kernel(const int32_t *__restrict__ ids, const float *__restrict__ dist, const int32_t *__restrict__ rows,
                                         int n, int k, int32_t *__restrict__ out_ids, float *__restrict__ out_dist) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (size_t)n * k; i += (size_t)gridDim.x * blockDim.x) {
    const size_t dst = (size_t)rows[i / k] * k + i % k;
    out_ids[dst] = ids[i];
    out_dist[dst] = dist[i];
  }
}

static bool is_host_pointer(const void *p) {
  hipPointerAttribute_t attr;
  hipError_t err = hipPointerGetAttributes(&attr, p);
  if (err != hipSuccess) {
    (void)hipGetLastError();  // clear
    return true;
  }
  return attr.type == hipMemoryTypeHost || attr.type == hipMemoryTypeUnregistered;
}

}  // namespace imp

using namespace imp;

struct imp_knn {
  size_t max_temp_memory = 0;
  // screened emit path: multiplier (1, 2, 4) of the threshold pre-pass's subset stride, steered by the candidate counts of the
  // previous batch of the same (catalogue size, k) -- see the feedback rule at emit_stride
  int stride_boost = 1;
  size_t boost_ni = 0;
  int boost_k = 0;
  // the per-query filter bitmap is all zeros between batches (every batch clears the words it set); true: not known to be (fresh
  // or regrown memory, a call that ended in an error) -- the next batch zeroes its part wholesale first
  bool row_bits_dirty = true;
  // persistent workspaces (grown on demand): no hipMalloc on the query path after the first call
  DeviceArray<float> scores, tile_max;
  DeviceArray<uint64_t> gcand;
  DeviceArray<int32_t> dev_ids, fallback;
  DeviceArray<float> dev_dist;
  // emit path
  DeviceArray<float> sub_scores, fb_query, fb_dist;
  DeviceArray<float> pad_items, pad_query;  // zero-padded fp32 copies for factor counts that are not a multiple of 16
  DeviceArray<split_bf16> query_split;      // [nq][3][f] bf16 (or [nq][2][f] fp16) terms of the query rows (emit path, split forms)
  // fp16 two-term form (topk_resident.h): the item matrix as fragment-ordered planes, made once per catalogue VERSION -- `key`
  // names the memory they were made from and is cleared by any write to it through the library (imp_matrix::mut_rows); memory the
  // library cannot vouch for (wrapped foreign pointers, matrices whose address was handed out) is split again on every call
  struct ItemPlanes {
    DerivedCache key;
    DeviceArray<_Float16> planes;
    DeviceArray<int> exp;          // scale exponent of the item matrix (from its exact maximum)
    DeviceArray<unsigned> maxbits;
    DeviceArray<unsigned> ne;      // bits of max || y 2^e ||_2, max || y 2^e - high plane ||_2, max ratio of the two (screened emit pass)
    DeviceArray<unsigned> tile_n;  // bits of max || y 2^e ||_2 per 32-item tile
    size_t rows = 0, cols = 0, itemsize = 0;
    int KS = 0;
    ItemPlanes() { register_derived_cache(&key); }
    ~ItemPlanes() { unregister_derived_cache(&key); }
  } item_planes;
  DeviceArray<_Float16> query_planes;
  DeviceArray<int> query_exp;
  DeviceArray<float> query_err;    // [2][rows]: || q 2^e - high plane ||, || high plane || per query row of the call
  DeviceArray<float> row_eps;
  DeviceArray<float> row_unscale;  // per row of an emit batch: what turns the raw accumulators its candidate keys carry into scores
  DeviceArray<uint32_t> tau, row_bits, item_bits;
  DeviceArray<unsigned int> cand_count;
  DeviceArray<uint64_t> cand;
  DeviceArray<int32_t> fb_rows, fb_ids;
  // page-locked, device-addressable host memory of the emit path: fallback flags and (host outputs) ids / scores are written
  // there by the kernels themselves (see OutputStage)
  struct Pinned {
    void *p = nullptr;
    size_t bytes = 0;
    void *ensure(size_t n) {
      if (bytes < n) {
        if (p) (void)hipHostFree(p);
        p = nullptr, bytes = 0;
        IMP_CHECK_HIP(hipHostMalloc(&p, n, hipHostMallocDefault));
        bytes = n;
      }
      return p;
    }
    ~Pinned() {
      if (p) (void)hipHostFree(p);
    }
  } host_stage;
};

namespace imp {
size_t knn_temp_budget(const imp_knn *k) { return k->max_temp_memory; }
}

// ---- host side of imp_knn_topk: checks -> operands -> outputs -> (emit | materialise) -> deliver ----------------------------
// The A/B and parity switches of the top-k entry point, read from the environment once per process.  Every route they select
// stays reachable: tests/test_gpu_topk_routes.py runs each of them.
struct TopkSwitches {
  bool fast;        // direct-operand MFMA GEMM (+ emit path, or tile maxima + single-pass pruned select); IMP_TOPK_NO_FAST set: general path
  bool emit;        // emit path (no score matrix); IMP_TOPK_NO_EMIT set: its shapes materialise their scores
  bool resident;    // fp16 two-term resident-query kernels; IMP_TOPK_RESIDENT=0: the six-product 128 x 128 kernel of rounds 3-4 (A/B, parity)
  bool screen;      // screened emit pass; IMP_TOPK_SCREEN=0: three products
  bool exact_mfma;  // IMP_TOPK_FP32_MFMA set: the exact-fp32 MFMA form (v_mfma_f32_32x32x2_f32) instead of the split-bf16 one (A/B, parity)
  bool debug;       // IMP_TOPK_DEBUG set: the rows every batch hands to the exact path, on stderr
};
static const TopkSwitches &topk_switches() {
  static const char *const resident = getenv("IMP_TOPK_RESIDENT"), *const screen = getenv("IMP_TOPK_SCREEN");
  static const TopkSwitches s{getenv("IMP_TOPK_NO_FAST") == nullptr, getenv("IMP_TOPK_NO_EMIT") == nullptr, !(resident && atoi(resident) == 0),
                              !(screen && atoi(screen) == 0), getenv("IMP_TOPK_FP32_MFMA") != nullptr, getenv("IMP_TOPK_DEBUG") != nullptr};
  return s;
}

// grid of a 256-thread grid-stride kernel over n elements: at most per_cu workgroups per compute unit
static int grid_1d(size_t n, int per_cu) { return (int)std::min<size_t>((n + 255) / 256, (size_t)ctx().num_cus * per_cu); }

// Where the kernels write a call's ids and scores, and how they reach the caller.
// Host outputs: the select kernels write ids and scores (and the emit path its fallback flags) STRAIGHT into page-locked
// host memory the device can address -- [2048 flags][2048 counts][ids of the call][scores of the call] -- and after the host
// wait they are simply there.  Any D2H copy instead costs more than the whole candidate sort: into pageable memory (the caller's
// numpy arrays) the runtime stages it with a host wait of its own (three per emit call: ~0.1 of a 0.59 ms call), and an
// ASYNCHRONOUS copy queued behind the kernels, page-locked or not, took ~0.4 ms to start on this stack (0.59 -> 1.0 ms
// per call, gpurun_out/r4o, r4q).  Very large results (> 64 MB per array) keep the device buffers and the copies.
constexpr size_t kFlagSlots = 2048;  // = query rows of an emit batch
struct OutputStage {
  int32_t *indices, *d_ids;  // the caller's array; what the kernels write: that array (device), its place in the page-locked stage or a device buffer
  float *distances, *d_dist;
  bool host_ids, host_dist, staged;
  size_t out_words;
  int *host_flags;   // emit path: one flag per row of the batch, read by the host after the batch's wait
  int *host_counts;  // screened select: the length of every row's candidate list (feeds the stride rule)
  void deliver() const {  // end of a call: wait, then hand the results over
    if (staged) {
      sync();
      if (host_ids) std::copy(d_ids, d_ids + out_words, indices);
      if (host_dist) std::copy(d_dist, d_dist + out_words, distances);
    } else {
      if (host_ids) IMP_CHECK_HIP(hipMemcpyAsync(indices, d_ids, out_words * 4, hipMemcpyDeviceToHost, stream()));
      if (host_dist) IMP_CHECK_HIP(hipMemcpyAsync(distances, d_dist, out_words * 4, hipMemcpyDeviceToHost, stream()));
      sync();
    }
  }
};
// a host output array's place in the stage, or a device buffer; `preset`: entries past k_eff keep the caller's initial values (topk.pyx:20-21)
template <typename T> static T *place_output(const OutputStage &o, const T *caller, T *stage, DeviceArray<T> &dev, bool preset) {
  if (o.staged) {
    if (preset) std::copy(caller, caller + o.out_words, stage);
    return stage;
  }
  T *d = dev.reserve(o.out_words);
  if (preset) IMP_CHECK_HIP(hipMemcpyAsync(d, caller, o.out_words * 4, hipMemcpyHostToDevice, stream()));
  return d;
}
static OutputStage stage_outputs(imp_knn *knn, size_t nq, int k, int k_eff, int32_t *indices, float *distances) {
  OutputStage o{indices, indices, distances, distances, is_host_pointer(indices), is_host_pointer(distances), false, nq * (size_t)k, nullptr, nullptr};
  o.staged = (o.host_ids || o.host_dist) && o.out_words <= ((size_t)16 << 20);
  o.host_flags = static_cast<int *>(knn->host_stage.ensure((2 * kFlagSlots + (o.staged ? 2 * o.out_words : 0)) * 4));
  o.host_counts = o.host_flags + kFlagSlots;
  int *stage = o.host_flags + 2 * kFlagSlots;
  if (o.host_ids) o.d_ids = place_output(o, indices, reinterpret_cast<int32_t *>(stage), knn->dev_ids, k_eff < k);
  if (o.host_dist) o.d_dist = place_output(o, distances, reinterpret_cast<float *>(stage + o.out_words), knn->dev_dist, k_eff < k);
  return o;
}

struct TopkCall {  // what a call computes once; every function below reads it
  imp_knn *knn;
  const imp_matrix *items_in;  // the item factors as the caller stored them (they name the cached item planes)
  size_t nq, ni;
  int f, k, k_eff, kpad;  // f: the factor count the kernels see (the caller's, or its zero-padded width on the 16-grid)
  bool fast;              // direct-operand MFMA GEMM; false: the general path (any f, any k: LDS-staged GEMM + exact select)
  bool use_lds;           // exact select: its kpad candidates fit in LDS
  int stride, n_tiles;    // emit path: every stride-th 128-item block is scored by the threshold pre-pass; 64-item tiles of a score row
  const float *norms;     // item norms (cosine scores) or null
  const imp_coo *query_filter;       // null: none, or empty
  const imp_intvector *item_filter;  // likewise
  OutputStage out;
};

// The factors as the kernels read them: as stored (fp32, or fp16 on the direct-operand kernels, which convert in registers --
// reference: SgemmEx on fp16 operands with fp32 accumulation, knn.cu:117-128), zero-padded fp32 copies in the handle's workspaces
// (factor counts off the 16-grid ride the fast path on them: 272 K -> 1.1 M recs/s at f = 100, configs[2] items; the copies cost
// ~0.1 ms per call at that size), or fp32 copies of fp16 factors (only the general path, any f, LDS-staged GEMM, scores those).
struct TopkOperands {
  const void *items, *query;
  bool half;                                           // both are fp16 as stored
  std::unique_ptr<imp_matrix> items_conv, query_conv;  // the converted copies live as long as the call
};
// factor counts that are not a multiple of 16 (the reference's CPU default is 100): rows zero-padded to the next multiple, fp16
// converted on the way -- extra zero factors change no dot product, and the scores come from the direct-operand kernels
template <typename T> static void pad_factors(const imp_matrix *m, float *out, int f) {
  pad_rows(std::max(1, grid_1d(m->rows * (size_t)f, 16)), m->as<T>(), out, m->rows, (int)m->cols, f);
}
static TopkOperands prepare_operands(imp_knn *knn, const imp_matrix *items_in, const imp_matrix *query_in, int f, bool fast) {
  TopkOperands op{items_in->as(), query_in->as(), items_in->itemsize == 2, nullptr, nullptr};
  if (f != (int)items_in->cols) {
    float *pi = knn->pad_items.reserve(items_in->rows * (size_t)f), *pq = knn->pad_query.reserve(query_in->rows * (size_t)f);
    IMP_PROF("pad_factors");
    if (op.half) pad_factors<__half>(items_in, pi, f), pad_factors<__half>(query_in, pq, f);
    else pad_factors<float>(items_in, pi, f), pad_factors<float>(query_in, pq, f);
    IMP_CHECK_HIP(hipGetLastError());
    op.items = pi, op.query = pq, op.half = false;
  } else if (op.half && !fast) {
    op.items_conv = astype(items_in, 4);
    op.query_conv = astype(query_in, 4);
    op.items = op.items_conv->as(), op.query = op.query_conv->as(), op.half = false;
  }
  return op;
}

// fp16 two-term planes for the resident-query kernels (topk_resident.h): the item matrix once per catalogue version (cached in
// the handle), the query rows of this call with one scale per row.  Returns the kernel arguments that name them, at query row 0
template <typename TQ, typename TI> static ResidentArgs split_planes(const TopkCall &c, int KS, const TQ *Qb, const TI *Ib) {
  IMP_PROF("split_query_rows");
  const imp_matrix *items_in = c.items_in;
  const size_t nq = c.nq, ni = c.ni, ni_pad = (ni + 127) / 128 * 128, F = (size_t)KS * 16;
  const int f = c.f;
  auto &ip = c.knn->item_planes;
  // (memory the library cannot vouch for never hits: the address may have been handed out after the planes were made)
  const bool same = ip.key.made_from(items_in) && ip.rows == ni && ip.cols == items_in->cols && ip.itemsize == items_in->itemsize && ip.KS == KS;
  if (!same) {
    IMP_PROF_NESTED("item_planes_split");  // one count per (re)build of the item planes: what the cache tests read
    ip.key.drop();
    ip.planes.reserve(ni_pad * F * 2), ip.exp.reserve(1), ip.maxbits.reserve(1), ip.ne.reserve(4), ip.tile_n.reserve(ni_pad / 32);
    IMP_CHECK_HIP(hipMemsetAsync(ip.maxbits.data(), 0, sizeof(unsigned), stream()));
    IMP_CHECK_HIP(hipMemsetAsync(ip.ne.data(), 0, 4 * sizeof(unsigned), stream()));
    IMP_CHECK_HIP(hipMemsetAsync(ip.tile_n.data(), 0, (ni_pad / 32) * sizeof(unsigned), stream()));
    rq_absmax_kernel<TI><<<std::max(1, grid_1d(ni * (size_t)f, 8)), 256, 0, stream()>>>(Ib, ni * (size_t)f, ip.maxbits.data());
    rq_item_exp_kernel<<<1, 1, 0, stream()>>>(ip.maxbits.data(), ip.exp.data());
    rq_split_items_kernel<TI><<<std::max(1, grid_1d(ni_pad * (F / 8), 16)), 256, 0, stream()>>>(Ib, ip.planes.data(), ni, ni_pad, f, KS, ip.exp.data());
    rq_item_err_kernel<TI><<<(int)std::min<size_t>((ni + 3) / 4, (size_t)ctx().num_cus * 16), 256, 0, stream()>>>(Ib, ni, f, ip.exp.data(),
                                                                                                              ip.ne.data(), ip.tile_n.data());
    ip.rows = ni, ip.cols = items_in->cols, ip.itemsize = items_in->itemsize, ip.KS = KS;
    ip.key.bind(items_in);
  }
  const size_t nq_pad = rq_query_pad(nq);
  _Float16 *qp = c.knn->query_planes.reserve(nq_pad * F * 2);
  int *qe = c.knn->query_exp.reserve(nq_pad);
  float *qerr = c.knn->query_err.reserve(2 * nq_pad);
  rq_split_queries_kernel<TQ><<<(int)std::min<size_t>((nq_pad + 3) / 4, (size_t)ctx().num_cus * 8), 256, 0, stream()>>>(Qb, qp, qe, nq, nq_pad, f, KS,
                                                                                                                       qerr, qerr + nq_pad);
  IMP_CHECK_HIP(hipGetLastError());
  ResidentArgs ra{};
  ra.qsplit = qp, ra.isplit = ip.planes.data(), ra.qexp = qe, ra.iexp = ip.exp.data(), ra.ni = (int)ni, ra.norms = c.norms;
  ra.qa = qerr, ra.qb = qerr + nq_pad, ra.ine = ip.ne.data(), ra.tile_n = reinterpret_cast<const float *>(ip.tile_n.data());
  return ra;
}

// a launch over `rows` query rows from `start`; the caller adds what its MODE writes (tile maxima or lists).  MODE 0 reads no qa .. tile_n / sub_cols
static ResidentArgs resident_args(ResidentArgs ra, int KS, size_t start, int rows, int n_blocks, int block_stride, float *S) {
  ra.qsplit += (start / 32) * (size_t)KS * 2 * 512, ra.qexp += start, ra.qa += start, ra.qb += start;
  ra.nq = rows, ra.n_blocks = n_blocks, ra.block_stride = block_stride, ra.S = S, ra.sub_cols = n_blocks * 128;
  return ra;
}

// the exact select of `rows` score rows (those flagged, or all); set_lds: the first launch of a loop sizes the kernel's LDS
static void launch_select_exact(const TopkCall &c, bool set_lds, const float *scores, int rows, int32_t *ids, float *dist, uint64_t *gcand, const int *flagged) {
  const size_t lds = c.use_lds ? (size_t)c.kpad * 8 : 0;
  auto kern = select_kernel<512>;
  if (set_lds)
    allow_dynamic_lds(kern, std::max<size_t>(lds, 1));
  kern<<<(unsigned)rows, 512, lds, stream()>>>(scores, (int)c.ni, c.k_eff, c.kpad, ids, dist, c.k, gcand, c.use_lds ? 1 : 0, flagged);
  IMP_CHECK_HIP(hipGetLastError());
}

// ---- emit path (no score matrix): large item sets, k small against the candidate lists ---------------------------------------
// one GEMM launch of a batch (MODE 1: subset scores, 2: three-product emit pass, 3: screened emit pass): on the resident planes
// (`planes`, else null), on query rows pre-split for the six-product kernel (`qs`, else null) or on the rows in their storage type
template <int M, typename TQ, typename TI, bool BF3>
static void emit_gemm(const TopkCall &c, const ResidentArgs *planes, int KS, const split_bf16 *qs, const TQ *Qb, const TI *Ib, size_t start, dim3 grid,
                      int rows, float *S_out, int bstride, const EmitArgs &ea) {
  if (planes) {
    ResidentArgs ra = resident_args(*planes, KS, start, rows, (int)grid.x, bstride, S_out);
    ra.emit = ea;
    launch_score_resident<M>(KS, ra, rows);
  } else if constexpr (M == 3) {
    throw std::logic_error("the screened emit pass exists in the resident form only");
  } else if (qs) {
    score_gemm_direct_kernel<M, split_bf16, TI, true><<<grid, 256, 0, stream()>>>(qs + start * 3 * (size_t)c.f, rows, Ib, (int)c.ni, c.f, c.norms, S_out,
                                                                            nullptr, 0, bstride, ea);
  } else {
    score_gemm_direct_kernel<M, TQ, TI, BF3><<<grid, 256, 0, stream()>>>(Qb + start * c.f, rows, Ib, (int)c.ni, c.f, c.norms, S_out, nullptr, 0, bstride, ea);
  }
}

static void clear_row_bits(const TopkCall &c, uint32_t *row_bits, size_t start, size_t end) {  // behind a batch: the words it set, back to zero
  const imp_coo *qf = c.query_filter;
  coo_bitmap_clear_kernel<<<grid_1d((size_t)qf->nnz, 8), 256, 0, stream()>>>(row_bits, (int)((c.ni + 31) / 32), (int)start, (int)end, (int)c.ni,
                                                                            qf->row.data(), qf->col.data(), (size_t)qf->nnz);
  IMP_CHECK_HIP(hipGetLastError());
  c.knn->row_bits_dirty = false;
}

static void scan_flags(const int *flags, size_t rows, std::vector<int32_t> &fb_list) {  // the rows a batch's select flagged for the exact path
  fb_list.clear();
  for (size_t i = 0; i < rows; ++i)
    if (flags[i]) fb_list.push_back((int32_t)i);
}

// the rows of the batch at `start` whose list overflowed, came up short or tied exactly at the k-th score: materialised FB rows at a time
template <typename TQ, typename TI, bool BF3>
static void emit_fallback_rows(const TopkCall &c, const TQ *qptr, const TI *Ib, size_t start, const std::vector<int32_t> &fb_list,
                               const uint32_t *row_bits, const uint32_t *item_bits) {
  IMP_PROF("topk_fallback");
  constexpr int FB = 64;  // fallback rows per materialised group
  imp_knn *knn = c.knn;
  const int ni = (int)c.ni, f = c.f, k = c.k, n_tiles = c.n_tiles;
  int32_t *d_rows = knn->fb_rows.reserve(fb_list.size());
  IMP_CHECK_HIP(hipMemcpyAsync(d_rows, fb_list.data(), fb_list.size() * 4, hipMemcpyHostToDevice, stream()));
  float *fbq = knn->fb_query.reserve((size_t)FB * f);
  float *fscores = knn->scores.reserve((size_t)FB * c.ni);
  float *ftile = knn->tile_max.reserve((size_t)FB * n_tiles);
  int32_t *fids = knn->fb_ids.reserve((size_t)FB * k);
  float *fdist = knn->fb_dist.reserve((size_t)FB * k);
  uint64_t *fg = c.use_lds ? nullptr : knn->gcand.reserve((size_t)FB * c.kpad);
  for (size_t g0 = 0; g0 < fb_list.size(); g0 += FB) {
    const int n = (int)std::min<size_t>(FB, fb_list.size() - g0);
    gather_query_rows_kernel<TQ><<<std::max(1, (n * f + 255) / 256), 256, 0, stream()>>>(qptr, d_rows + g0, n, f, fbq);
    score_gemm_direct_kernel<0, float, TI, BF3><<<dim3((unsigned)((c.ni + 127) / 128), 1), 256, 0, stream()>>>(fbq, n, Ib, ni, f, c.norms, fscores, ftile,
                                                                                                           n_tiles, 1, EmitArgs{});
    if (row_bits || item_bits)
      bitmap_filter_kernel<<<grid_1d((size_t)n * n_tiles, 8), 256, 0, stream()>>>(fscores, ftile, ni, n_tiles, d_rows + g0, n, row_bits, item_bits,
                                                                                 (int)((c.ni + 31) / 32));
    launch_select_exact(c, g0 == 0, fscores, n, fids, fdist, fg, nullptr);
    scatter_topk_rows_kernel<<<std::max(1, (n * k + 255) / 256), 256, 0, stream()>>>(fids, fdist, d_rows + g0, n, k, c.out.d_ids + start * k,
                                                                                 c.out.d_dist + start * k);
    IMP_CHECK_HIP(hipGetLastError());
  }
}

template <typename TQ, typename TI, bool BF3> static void emit_route(const TopkCall &c, const TQ *Qb, const TI *Ib) {
  imp_knn *knn = c.knn;
  const TopkSwitches &sw = topk_switches();
  const size_t nq = c.nq, ebatch = std::min<size_t>(nq, kFlagSlots);  // (one flag per row of a batch)
  const int ni = (int)c.ni, f = c.f, k = c.k, k_eff = c.k_eff, stride = c.stride;
  const imp_coo *qf = c.query_filter;
  const imp_intvector *itf = c.item_filter;
  const int words = (int)((c.ni + 31) / 32), n_blocks = (int)((c.ni + 127) / 128), n_sub = (n_blocks + stride - 1) / stride, sub_cols = n_sub * 128;
  float *sub = knn->sub_scores.reserve(ebatch * (size_t)sub_cols);
  uint32_t *tau = knn->tau.reserve((ebatch + 127) / 128 * 128);  // the emit epilogue loads thresholds four rows at a time
  unsigned int *cnt = knn->cand_count.reserve(ebatch);
  uint64_t *cand = knn->cand.reserve(ebatch * (size_t)kEmitCap);
  float *row_unscale = knn->row_unscale.reserve(rq_query_pad(ebatch));
  int *flags = c.out.host_flags, *list_len = c.out.host_counts;
  if (qf && knn->row_bits.size < ebatch * (size_t)words) knn->row_bits_dirty = true;  // (about to be regrown: fresh memory)
  uint32_t *row_bits = qf ? knn->row_bits.reserve(ebatch * (size_t)words) : nullptr;
  uint32_t *item_bits = itf ? knn->item_bits.reserve((size_t)words) : nullptr;
  if (itf) IMP_CHECK_HIP(hipMemsetAsync(item_bits, 0, (size_t)words * 4, stream()));
  // fp16 two-term form with the queries resident in registers and the item planes cached (topk_resident.h): every factor count
  // that pads to 32 / 64 / 128 / 256; fp16-stored factors too (their values are their own high halves: scores stay bit-identical
  // to scoring fp32 copies of them).  IMP_TOPK_RESIDENT=0: the six-product 128 x 128 kernel of rounds 3-4 (A/B, parity)
  const int KS = rq_ks_for(f);
  const bool resident = BF3 && sw.resident && KS > 0;
  ResidentArgs plane_args{};
  split_bf16 *qs = nullptr;
  if (resident) {
    plane_args = split_planes(c, KS, Qb, Ib);
  } else if (BF3) {
    IMP_PROF("split_query_rows");
    const size_t nq_pad = (nq + 127) / 128 * 128;  // whole 128-row query blocks: a workgroup reads all four tiles of its block
    qs = knn->query_split.reserve(nq_pad * 3 * (size_t)f);
    split_query_rows_kernel<TQ><<<std::max(1, grid_1d(nq_pad * (size_t)f, 16)), 256, 0, stream()>>>(Qb, reinterpret_cast<__bf16 *>(qs), nq, nq_pad, f);
    IMP_CHECK_HIP(hipGetLastError());
  }
  const ResidentArgs *planes = resident ? &plane_args : nullptr;
  float *unscale = resident ? row_unscale : nullptr;
  // screened emit pass (topk_resident.h MODE 3): one-product scores against tau - eps, the few candidates that can still be among
  // the best k re-scored in fp32 by the select kernel.  Dot-product scores only (no item norms); IMP_TOPK_SCREEN=0: three products
  const bool screen = resident && sw.screen && !c.norms;
  float *row_eps = screen ? knn->row_eps.reserve(rq_query_pad(ebatch)) : nullptr;
  std::vector<int32_t> fb_list;
  for (size_t start = 0; start < nq; start += ebatch) {
    const size_t end = std::min(nq, start + ebatch), rows = end - start;
    const dim3 sub_grid((unsigned)n_sub, (unsigned)((rows + 127) / 128)), full_grid((unsigned)n_blocks, (unsigned)((rows + 127) / 128));
    int32_t *ids = c.out.d_ids + start * k;
    float *dist = c.out.d_dist + start * k;
    if (qf) {
      if (knn->row_bits_dirty) IMP_CHECK_HIP(hipMemsetAsync(row_bits, 0, knn->row_bits.size * sizeof(uint32_t), stream()));
      knn->row_bits_dirty = true;  // (until this batch's clear is queued)
    }
    {
      IMP_PROF("score_gemm_subset");
      emit_gemm<1, TQ, TI, BF3>(c, planes, KS, qs, Qb, Ib, start, sub_grid, (int)rows, sub, stride, EmitArgs{});
      IMP_CHECK_HIP(hipGetLastError());
    }
    if (itf) {
      IMP_PROF("item_filter");
      item_bitmap_kernel<<<grid_1d(itf->size, 8), 256, 0, stream()>>>(item_bits, ni, itf->v.data(), (int)itf->size, sub, (int)rows, sub_cols, stride);
      IMP_CHECK_HIP(hipGetLastError());
    }
    if (qf) {
      IMP_PROF("coo_filter");
      coo_bitmap_kernel<<<grid_1d((size_t)qf->nnz, 8), 256, 0, stream()>>>(row_bits, words, (int)start, (int)end, ni, qf->row.data(), qf->col.data(),
                                                                          (size_t)qf->nnz, sub, sub_cols, stride);
      IMP_CHECK_HIP(hipGetLastError());
    }
    {
      IMP_PROF("topk_threshold");
      if (k_eff <= 32) subset_threshold_groupmax_kernel<256><<<(unsigned)rows, 256, 0, stream()>>>(sub, sub_cols, k_eff, tau, cnt);
      else subset_threshold_kernel<512><<<(unsigned)rows, 512, 0, stream()>>>(sub, sub_cols, k_eff, tau, cnt);
      IMP_CHECK_HIP(hipGetLastError());
    }
    {
      IMP_PROF("score_gemm");
      EmitArgs ea{tau, row_bits, item_bits, words, cand, cnt, kEmitCap, unscale, row_eps};
      if (screen) emit_gemm<3, TQ, TI, BF3>(c, planes, KS, qs, Qb, Ib, start, full_grid, (int)rows, nullptr, 1, ea);
      else emit_gemm<2, TQ, TI, BF3>(c, planes, KS, qs, Qb, Ib, start, full_grid, (int)rows, nullptr, 1, ea);
      IMP_CHECK_HIP(hipGetLastError());
    }
    {
      IMP_PROF("topk_select_candidates");
      if (screen)
        select_screened_kernel<512, TQ, TI><<<(unsigned)rows, 512, 0, stream()>>>(cand, cnt, kEmitCap, k_eff, ids, dist, k, flags, row_eps, Qb + start * f,
                                                                                 Ib, f, list_len);
      else
        select_candidates_kernel<512><<<(unsigned)rows, 512, 0, stream()>>>(cand, cnt, kEmitCap, k_eff, ids, dist, k, flags, unscale);
      IMP_CHECK_HIP(hipGetLastError());
#ifdef RQ_SCREEN_STATS
      if (screen) {
        unsigned long long h[4];
        IMP_CHECK_HIP(hipStreamSynchronize(stream()));
        IMP_CHECK_HIP(hipMemcpyFromSymbol(h, HIP_SYMBOL(rq_screen_stats), sizeof(h)));
        fprintf(stderr, "[screen-stats] rows %llu, candidates per row %.1f, re-scored per row %.1f (largest so far: %llu)\n", h[0],
                (double)h[1] / std::max(1ull, h[0]), (double)h[2] / std::max(1ull, h[0]), h[3]);
      }
#endif
    }
    sync();
    scan_flags(flags, rows, fb_list);
    if (screen && fb_list.size() * 8 > rows) {
      // The screen separated nothing for much of this batch: scores so concentrated that an 11-bit product cannot tell the
      // best k from the bulk (factors a sweep or two from an all-positive start: every score within 1e-3 of the next) -- the
      // lists overflowed.  The WHOLE batch is redone by the three-product emit pass with its exact threshold test (same
      // thresholds, lists reset) before anything goes to the row-by-row exact path: 0.25 ms per 1000 rows instead of 1.3.
      // Decided by this batch's own outcome, not by the handle's history: the same call gives the same bits every time.
      IMP_PROF("topk_exact_emit_retry");
      IMP_CHECK_HIP(hipMemsetAsync(cnt, 0, rows * sizeof(unsigned int), stream()));
      EmitArgs ea{tau, row_bits, item_bits, words, cand, cnt, kEmitCap, row_unscale, nullptr};
      emit_gemm<2, TQ, TI, BF3>(c, planes, KS, qs, Qb, Ib, start, full_grid, (int)rows, nullptr, 1, ea);
      select_candidates_kernel<512><<<(unsigned)rows, 512, 0, stream()>>>(cand, cnt, kEmitCap, k_eff, ids, dist, k, flags, row_unscale);
      IMP_CHECK_HIP(hipGetLastError());
      sync();
      scan_flags(flags, rows, fb_list);
    }
    if (screen && rows >= 64) {  // the stride rule (emit_stride): mean list length and exact-path rows of this batch
      size_t total = 0;
      for (size_t i = 0; i < rows; ++i) total += (size_t)list_len[i];
      const size_t mean = total / rows;
      if (fb_list.size() * 100 > rows || mean > 400) knn->stride_boost = std::max(1, knn->stride_boost / 2);
      else if (mean < 48 && knn->stride_boost < 4) knn->stride_boost *= 2;
    }
    if (sw.debug && !fb_list.empty()) {
      std::vector<uint32_t> hc(rows), ht(rows);
      IMP_CHECK_HIP(hipMemcpy(hc.data(), cnt, rows * 4, hipMemcpyDeviceToHost));
      IMP_CHECK_HIP(hipMemcpy(ht.data(), tau, rows * 4, hipMemcpyDeviceToHost));
      fprintf(stderr, "[topk-debug] batch at %zu: %zu fallback rows:", start, fb_list.size());
      for (size_t i = 0; i < std::min<size_t>(fb_list.size(), 8); ++i)
        fprintf(stderr, " (row %d count %u tau-key %08x)", fb_list[i], hc[fb_list[i]], ht[fb_list[i]]);
      fprintf(stderr, "\n");
    }
    if (!fb_list.empty()) emit_fallback_rows<TQ, TI, BF3>(c, Qb + start * f, Ib, start, fb_list, row_bits, item_bits);
    if (qf && end < nq) clear_row_bits(c, row_bits, start, end);  // (the last batch's: behind the call's wait, below)
  }
  c.out.deliver();
  if (qf) clear_row_bits(c, row_bits, (nq - 1) / ebatch * ebatch, nq);
}

// ---- materialising path: a batch of score rows, the filters on them, pruned select, exact select of the rows it flagged --------
template <typename TQ, typename TI, bool BF3> static void materialise_route(const TopkCall &c, const TQ *Qb, const TI *Ib) {
  imp_knn *knn = c.knn;
  const int ni = (int)c.ni, f = c.f, k = c.k, n_tiles = c.n_tiles;
  const bool fast = c.fast;
  const imp_coo *qf = c.query_filter;
  const imp_intvector *itf = c.item_filter;
  const size_t nq = c.nq, temp = std::min<size_t>(knn->max_temp_memory, (size_t)4 << 30);
  size_t batch = std::max<size_t>(1, std::min<size_t>(nq, temp / (sizeof(float) * c.ni)));
  // a resident launch reads whole 128-row blocks of query planes from its first row on: batches start on that grid, or use the direct kernel
  const int KS = rq_ks_for(f);
  const bool resident = BF3 && fast && topk_switches().resident && KS > 0 && (batch == nq || batch >= 128);
  if (resident && batch < nq) batch = batch / 128 * 128;
  float *scores = knn->scores.reserve(batch * c.ni);
  uint64_t *gcand = c.use_lds ? nullptr : knn->gcand.reserve(batch * (size_t)c.kpad);
  float *tile_max = fast ? knn->tile_max.reserve(batch * (size_t)n_tiles) : nullptr;
  int *fallback = fast ? knn->fallback.reserve(batch) : nullptr;
  const ResidentArgs planes = resident ? split_planes(c, KS, Qb, Ib) : ResidentArgs{};
  for (size_t start = 0; start < nq; start += batch) {
    const size_t end = std::min(nq, start + batch), rows = end - start;
    int32_t *ids = c.out.d_ids + start * k;
    float *dist = c.out.d_dist + start * k;
    if (resident) {
      IMP_PROF("score_gemm");
      ResidentArgs ra = resident_args(planes, KS, start, (int)rows, (int)((c.ni + 127) / 128), 1, scores);
      ra.tile_max = tile_max, ra.n_tiles64 = n_tiles;
      launch_score_resident<0>(KS, ra, (int)rows);
    } else if (fast) {
      IMP_PROF("score_gemm");
      dim3 grid((unsigned)((c.ni + 127) / 128), (unsigned)((rows + 127) / 128));
      score_gemm_direct_kernel<0, TQ, TI, BF3><<<grid, 256, 0, stream()>>>(Qb + start * f, (int)rows, Ib, ni, f, c.norms, scores, tile_max, n_tiles, 1,
                                                                          EmitArgs{});
      IMP_CHECK_HIP(hipGetLastError());
    } else {
      IMP_PROF("score_gemm_lds");
      dim3 grid((unsigned)((c.ni + kBN - 1) / kBN), (unsigned)((rows + kBM - 1) / kBM));
      if constexpr (std::is_same<TQ, float>::value) {  // the general path always runs on fp32 (copies of fp16 factors)
        score_gemm_kernel<<<grid, 256, 0, stream()>>>(Qb + start * f, (int)rows, Ib, ni, f, c.norms, scores);
        IMP_CHECK_HIP(hipGetLastError());
      }
    }
    if (itf) {
      IMP_PROF("item_filter");
      item_filter_kernel<<<grid_1d(rows * itf->size, 8), 256, 0, stream()>>>(scores, (int)rows, ni, itf->v.data(), (int)itf->size);
      IMP_CHECK_HIP(hipGetLastError());
    }
    if (qf) {
      IMP_PROF("coo_filter");
      coo_filter_kernel<<<grid_1d((size_t)qf->nnz, 8), 256, 0, stream()>>>(scores, (int)start, (int)end, ni, qf->row.data(), qf->col.data(), (size_t)qf->nnz);
      IMP_CHECK_HIP(hipGetLastError());
    }
    if (fast && (itf || qf)) {
      // second phase (all filter writes are done): refresh the maxima of the touched tiles
      IMP_PROF("filter_tile_refresh");
      if (itf)
        item_filter_refresh_kernel<<<grid_1d(rows * itf->size, 8), 256, 0, stream()>>>(scores, tile_max, (int)rows, ni, n_tiles, itf->v.data(), (int)itf->size);
      if (qf)
        coo_filter_refresh_kernel<<<grid_1d((size_t)qf->nnz, 8), 256, 0, stream()>>>(scores, tile_max, (int)start, (int)end, ni, n_tiles, qf->row.data(),
                                                                                    qf->col.data(), (size_t)qf->nnz);
      IMP_CHECK_HIP(hipGetLastError());
    }
    if (fast) {
      IMP_PROF("topk_select_pruned");
      // (extra = 0, filter_counts = null: the tile maxima are refreshed after the filters, so no slack for filtered entries is needed)
      select_pruned_kernel<512><<<(unsigned)rows, 512, 0, stream()>>>(scores, tile_max, ni, n_tiles, c.k_eff, 0, nullptr, ids, dist, k, fallback);
      IMP_CHECK_HIP(hipGetLastError());
    }
    {
      IMP_PROF("topk_select");
      launch_select_exact(c, true, scores, (int)rows, ids, dist, gcand, fallback);
    }
    if (topk_switches().debug && fast) {  // how many rows the pruned select handed to the exact select
      std::vector<int> hf(rows);
      IMP_CHECK_HIP(hipMemcpy(hf.data(), fallback, rows * sizeof(int), hipMemcpyDeviceToHost));
      size_t nfb = 0, first_fb = 0;
      for (size_t i = rows; i-- > 0;)
        if (hf[i]) first_fb = i, ++nfb;
      fprintf(stderr, "[topk-debug] materialising batch at %zu: %zu of %zu rows re-done by the exact select (first: row %zu)\n", start, nfb, rows, first_fb);
    }
  }
  c.out.deliver();
}

// The stride of the emit path's threshold pre-pass.  The emit path pays when the candidate lists stay SPARSE: every `stride`-th 128-item block is scored first and
// about stride x k entries per query survive its threshold.  The stride is chosen so that they fill at most half of a
// query's kEmitCap slots AND are at most one in 64 of the items -- every 64-item tile with a survivor costs an atomic on
// the query's counter and a scattered store (measured at configs[4]'s similar_items shape, 26 744 items, k = 100,
// stride 20: 7.5 % of all scores survive and the emit GEMM runs at 10 TFLOP/s against 33 for the materialising path) --
// and a stride below 8 (a pre-pass of more than an eighth of the GEMM) is not worth it either.
// The stride is a trade between the pre-pass (scores of 1 / stride of the items materialised, filtered, selected from) and the
// candidate lists (about stride x k entries on unstructured data).  On TRAINED factors a row's best scores stand far above the
// bulk and the lists stay short (22 entries at stride 32 on the bench's factors), so the screened path lets the stride grow:
// after every batch the mean list length decides -- under 48: twice the stride next time (up to 4 x 32), over 400 or more than
// one row in a hundred sent to the exact path: half.  Results do not depend on the stride; random factors stay at 32
// (stride 128 there: 1280-entry lists and every row's staging overflowing -- measured, profiles/r06_topk_resident_knockouts.txt).
static int emit_stride(imp_knn *knn, size_t ni, int k_eff, bool cosine) {
  if (knn->boost_ni != ni || knn->boost_k != k_eff) knn->stride_boost = 1, knn->boost_ni = ni, knn->boost_k = k_eff;
  const int stride_cap = cosine ? kSubStride : kSubStride * knn->stride_boost;
  return (int)std::min<size_t>(std::min(stride_cap, kEmitCap / (2 * std::max(1, k_eff))), ni / ((size_t)64 * std::max(1, k_eff)));
}

template <typename T, bool BF3> static void topk_route(const TopkCall &c, bool emit, const TopkOperands &op) {
  const T *Qb = static_cast<const T *>(op.query), *Ib = static_cast<const T *>(op.items);
  emit ? emit_route<T, T, BF3>(c, Qb, Ib) : materialise_route<T, T, BF3>(c, Qb, Ib);
}

extern "C" {

int imp_knn_create(size_t max_temp_memory, imp_knn **out) {
  return guarded([&] {
    (void)ctx();
    if (!max_temp_memory) {
      size_t free_b = 0, total_b = 0;
      IMP_CHECK_HIP(hipMemGetInfo(&free_b, &total_b));
      max_temp_memory = std::min<size_t>(free_b / 2, (size_t)4 << 30);
    }
    auto k = new imp_knn();
    k->max_temp_memory = max_temp_memory;
    *out = k;
  });
}

int imp_knn_destroy(imp_knn *k) {
  return guarded([&] { delete k; });
}

int imp_knn_topk(imp_knn *knn, const imp_matrix *items_in, const imp_matrix *query_in, int k, int32_t *indices, float *distances,
                 const imp_matrix *item_norms, const imp_coo *query_filter, const imp_intvector *item_filter) {
  return guarded([&] {
    if (query_in->cols != items_in->cols) throw std::invalid_argument("Must have same number of columns in each matrix for topk");
    if (query_in->itemsize != items_in->itemsize) throw std::invalid_argument("Must have same dtype in each matrix for topk");
    if (k < 0) throw std::invalid_argument("k must be >= 0 for topk");
    if (item_norms && (item_norms->itemsize != 4 || item_norms->rows * item_norms->cols != items_in->rows))
      throw std::invalid_argument("item_norms must be a float32 matrix with one entry per item");
    const size_t nq = query_in->rows, ni = items_in->rows;
    const int f_in = (int)items_in->cols;
    if (nq == 0 || k == 0) return;
    if (ni > (size_t)INT32_MAX) throw std::invalid_argument("too many items for topk");
    const TopkSwitches &sw = topk_switches();
    const int k_eff = (int)std::min<size_t>((size_t)k, ni);
    const bool padded = sw.fast && f_in % 16 != 0 && f_in >= 1 && k_eff <= kCandCap;  // (see TopkOperands)
    const int f = padded ? (f_in + 15) / 16 * 16 : f_in;
    const bool fast = sw.fast && (f % 8 == 0) && k_eff <= kCandCap;
    const TopkOperands op = prepare_operands(knn, items_in, query_in, f, fast);
    int kpad = 1;
    while (kpad < k_eff) kpad <<= 1;
    if (kpad < 2) kpad = 2;
    const OutputStage out = stage_outputs(knn, nq, k, k_eff, indices, distances);
    const int stride = emit_stride(knn, ni, k_eff, item_norms != nullptr);
    const TopkCall c{knn, items_in, nq, ni, f, k, k_eff, kpad, fast, (size_t)kpad * 8 <= 96 * 1024, stride,
                     (int)((ni + kTileItems - 1) / kTileItems), item_norms ? item_norms->f32() : nullptr,
                     query_filter && query_filter->nnz ? query_filter : nullptr, item_filter && item_filter->size ? item_filter : nullptr, out};
    // ONE predicate decides both what is allocated (the emit route has no score matrix) and what runs
    const bool emit = fast && sw.emit && k_eff == k && k_eff <= 256 && stride >= 8;
    // split-bf16 / two-term forms need f on the 16-grid -- and every f of the fast path is: one that is not was padded above
    const bool bf3 = fast && !sw.exact_mfma;
    if (op.half) bf3 ? topk_route<__half, true>(c, emit, op) : topk_route<__half, false>(c, emit, op);
    else bf3 ? topk_route<float, true>(c, emit, op) : topk_route<float, false>(c, emit, op);
  });
}

}  // extern "C"
