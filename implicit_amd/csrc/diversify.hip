// K23: diversified re-ranking of per-user candidate lists: greedy MAP inference of a determinantal point process
// (Chen, Zhang, Zhou, NeurIPS 2018) and maximal marginal relevance (Carbonell & Goldstein, 1998).  NEW: the reference has
// neither.
//
// Candidate i of a list has the stored item row y_i and a quality q_i.  DPP: L = B B^T with b_i = q_i y_i / |y_i|; the greedy
// is column-pivoted Gram-Schmidt on the rows of B (the header states it step by step).  MMR: the value of candidate i is
// lambda q_i - (1 - lambda) max over the picks j of cos(y_i, y_j).  Both are one loop: pick the largest key, form the step's
// vector u (DPP: the pivot's row orthogonalised twice against the basis and normalised; MMR: the pivot's unit row), then
// e_i = s_i <y_i, u> for EVERY candidate (s_i = q_i / |y_i|, or 1 / |y_i|) and d2_i -= e_i^2, or max_i = max(max_i, e_i).
//
// One workgroup per list.  A candidate belongs to a group of G lanes (a power of two, 1 .. 64), lane g of the group holding the
// CPL consecutive columns from g CPL on; G and CPL follow from the width alone.  Group `grp` of the workgroup owns the
// candidates grp, grp + groups, ...
//   resident  (CPT >= 1) the lane keeps its columns of CPT candidates in registers (CPL x CPT floats, 16 or 64) for all steps:
//             lists up to 1024 x 64 / (G CPL) candidates, 512 at w = 128 (CPL = 4, w <= 32: half that);
//   streamed  (CPT == 0) the lane loads them from the item matrix again in every step (lists past the register budget).
// Either way e_i is dot_cols() -- one fmaf chain over the lane's columns, then the xor butterfly of group_allsum -- on the same
// operands, so a list gives the same bytes on either path, with any block size, in any batch or chunk.
// Per candidate the LDS holds five words (value, scale, quality, norm, id; a picked or padding candidate has a negative id),
// read and written by lane 0 of the owning group only.  The pivot's own row is formed as the header states it, q_j (y_j / |y_j|).
// The step's vector, the coefficients and (where it fits) the basis are in the LDS as well; a basis too large for it (min(n, w)
// rows of G CPL floats) goes to a device scratch of the workgroup's own.
// Barriers per step: DPP 3 for the first pick and 7 after it (winner slots; pivot row; 2 x (coefficients, subtraction); the
// new basis row), MMR 2 (winner slots; pivot row).  No floating-point atomic, no atomic at all.
#include <hip/hip_fp16.h>

#include <algorithm>
#include <cfloat>
#include <cmath>

#include "common.h"
#include "select_ops.h"
#include "wave_ops.h"

namespace imp {

constexpr int kDivBlock = 1024;       // most threads of a workgroup: 16 wavefronts, 128 registers each
constexpr int kDivMaxList = 4096;     // longest list
constexpr int kDivMaxWidth = 1024;    // most stored columns
// floats of candidate rows a lane keeps in registers on the resident path: the small form, and the full form for lists up to
// four times (CPL = 4: twice) as long.  64 floats at CPL = 8 / 16 compile to 119 / 116 registers of the 128 a wavefront of a
// 1024-thread workgroup has; 16 candidates of 4 columns spill (12 bytes), so the narrow widths stop at 8 candidates per lane.
constexpr int kDivFragSmall = 16;
constexpr int div_frag_full(int cpl) { return cpl == 4 ? 32 : 64; }
constexpr size_t kDivLdsLimit = 128 << 10;  // state + vectors + basis of one workgroup; a larger basis goes to the device scratch
constexpr int kDivSlotWords = 48;     // 16 winner keys (64 bit) and 16 winner positions, ahead of the arrays

__device__ __forceinline__ float div_widen(float v) { return v; }
__device__ __forceinline__ float div_widen(__half v) { return __half2float(v); }

// Sum over an aligned group of g lanes (a power of two), in every lane of the group: the xor butterfly of group_allsum
// (wave_ops.h), cut off at the group's size.  Every lane of the wavefront must be active.
__device__ __forceinline__ float div_group_sum(float v, int g) {
  if (g >= 2) v += dpp_mov<0xB1>(v);   // quad_perm [1,0,3,2]
  if (g >= 4) v += dpp_mov<0x4E>(v);   // quad_perm [2,3,0,1]
  if (g >= 8) v += dpp_mov<0x141>(v);  // row_half_mirror
  if (g >= 16) v += dpp_mov<0x140>(v);  // row_mirror
  if (g >= 32) v += __shfl_xor(v, 16);
  if (g >= 64) v += __shfl_xor(v, 32);
  return v;
}

// <a, b> over the group's columns: THE instruction sequence of a candidate's e on both paths
template <int CPL> __device__ __forceinline__ float dot_cols(const float (&a)[CPL], const float (&b)[CPL], int g) {
  float acc = 0.f;
#pragma unroll
  for (int c = 0; c < CPL; ++c) acc = fmaf(a[c], b[c], acc);
  return div_group_sum(acc, g);
}

// the lane's columns of one stored row, widened; zeros past the width and for no row at all
template <typename TI, int CPL> __device__ __forceinline__ void load_cols(const TI *row, int col0, int w, float (&y)[CPL]) {
#pragma unroll
  for (int c = 0; c < CPL; ++c) y[c] = (row && col0 + c < w) ? div_widen(row[col0 + c]) : 0.f;
}

struct DivShape {
  int g;        // lanes per candidate
  int m_cap;    // candidate slots of the LDS state: a multiple of the groups per workgroup, >= the longest list
  int k_cap;    // basis rows (DPP), 0 for MMR
  int lds_basis;  // the basis lives in the LDS
};

// offsets hold the chunk's rows + 1 entries, relative to the chunk's first candidate.
template <typename TI, int CPL, int CPT>
__global__ __launch_bounds__(kDivBlock) void diversify_kernel(const TI *__restrict__ items, int w, DivShape shape,
                                                             const int64_t *__restrict__ offsets, const int32_t *__restrict__ cand,
                                                             const float *__restrict__ quality, int n, int rule, float lambda,
                                                             float min_gain, float *basis_scratch, int32_t *__restrict__ ids_out,
                                                             float *__restrict__ gains_out, int32_t *__restrict__ counts_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned int div_lds[];
  const int G = shape.g, m_cap = shape.m_cap, k_cap = shape.k_cap, w_pad = G * CPL;
  uint64_t *slot_key = reinterpret_cast<uint64_t *>(div_lds);          // [16]
  int *slot_pos = reinterpret_cast<int *>(div_lds + 32);               // [16]
  float *val = reinterpret_cast<float *>(div_lds + kDivSlotWords);     // [m_cap] DPP: d2_i; MMR: the running maximum
  float *scale = val + m_cap;                                          // [m_cap] s_i
  float *rel = scale + m_cap;                                          // [m_cap] q_i
  float *nrm = rel + m_cap;                                            // [m_cap] |y_i|
  int *cid = reinterpret_cast<int *>(nrm + m_cap);                     // [m_cap] id; ~id once picked; -1 past the list
  float *rvec = reinterpret_cast<float *>(cid + m_cap);                // [w_pad] the pivot's row, then the step's residual
  float *coef = rvec + w_pad;                                          // [k_cap]
  float *U = shape.lds_basis ? coef + k_cap : basis_scratch + (size_t)blockIdx.x * k_cap * w_pad;  // [k_cap][w_pad]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, threads = blockDim.x, waves = threads >> 6;
  const int gl = tid & (G - 1), grp = tid / G, groups = threads / G, col0 = gl * CPL;
  const size_t r = blockIdx.x;
  const int64_t begin = offsets[r];
  const int len = (int)(offsets[r + 1] - begin);
  const int32_t *c = cand + begin;
  const float *q = quality + begin;
  const float one_minus = 1.f - lambda;

  // ---- the rows, and the state of every slot -------------------------------------------------------------------------------
  auto init = [&](int i, const float(&y)[CPL]) {
    const float n2 = dot_cols<CPL>(y, y, G);
    if (gl == 0 && i < m_cap) {
      const bool live = i < len;
      const float qi = live ? q[i] : 0.f, norm = sqrtf(n2);
      const float s = norm > 0.f ? (rule == 0 ? qi : 1.f) / norm : 0.f;
      scale[i] = s;
      rel[i] = qi;
      nrm[i] = norm;
      val[i] = rule == 0 ? (s * s) * n2 : 0.f;
      cid[i] = live ? c[i] : -1;
    }
  };
  float frag[CPT > 0 ? CPT : 1][CPL];
  if constexpr (CPT > 0) {
#pragma unroll
    for (int t = 0; t < CPT; ++t) {
      const int i = t * groups + grp;
      load_cols<TI, CPL>(i < len ? items + (size_t)c[i] * w : nullptr, col0, w, frag[t]);
      init(i, frag[t]);
    }
  } else {
    for (int i0 = 0; i0 < m_cap; i0 += groups) {
      const int i = i0 + grp;
      float y[CPL];
      load_cols<TI, CPL>(i < len ? items + (size_t)c[i] * w : nullptr, col0, w, y);
      init(i, y);
    }
  }

  int count = 0;
  for (int k = 0; k < n; ++k) {
    // ---- 1. the largest key: (value desc, id desc, position desc) -----------------------------------------------------------
    uint64_t best = 0;
    int bpos = -1;
    if (gl == 0) {
      for (int i = grp; i < m_cap; i += groups) {
        const int id = cid[i];
        if (id < 0) continue;
        const float v = rule == 0 ? val[i] : lambda * rel[i] - one_minus * val[i];
        const uint64_t key = make_key(v, id);
        if (key >= best) best = key, bpos = i;
      }
    }
    {
      const uint32_t hi = (uint32_t)(best >> 32), lo = (uint32_t)best;
      const uint32_t mh = wave_allmax_u32(hi);
      const uint32_t ml = wave_allmax_u32(hi == mh ? lo + 1u : 0u);
      const uint32_t mp = wave_allmax_u32(hi == mh && lo + 1u == ml ? (uint32_t)(bpos + 1) : 0u);
      if (lane == 0) {
        slot_key[wave] = ((uint64_t)mh << 32) | (ml - 1u);
        slot_pos[wave] = (int)mp - 1;
      }
    }
    __syncthreads();
    best = 0, bpos = -1;
    for (int v = 0; v < waves; ++v) {
      const uint64_t key = slot_key[v];
      const int pos = slot_pos[v];
      if (pos >= 0 && (key > best || (key == best && pos > bpos))) best = key, bpos = pos;
    }
    if (bpos < 0) break;  // the list is used up

    // ---- 2. the step's vector ---------------------------------------------------------------------------------------------------
    const int j = bpos, idj = cid[j];
    const float nj = nrm[j], qj = rel[j], vj = val[j];
    const TI *yj = items + (size_t)idj * w;
    for (int x = tid; x < w_pad; x += threads) {  // b_j = q_j (y_j / |y_j|), or the unit row; a zero row stays zero
      const float unit = x < w && nj > 0.f ? div_widen(yj[x]) / nj : 0.f;
      rvec[x] = rule == 0 ? qj * unit : unit;
    }
    __syncthreads();
    if (gl == 0 && grp == j % groups) cid[j] = ~idj;  // every thread has read it
    float gain;
    const float *u = rvec;
    if (rule == 0) {
      if (count >= k_cap) break;  // rank(B) <= w picks are made
      for (int pass = 0; pass < 2 && count > 0; ++pass) {  // classical Gram-Schmidt, twice
        for (int l = wave; l < count; l += waves) {
          float acc = 0.f;
          for (int x = lane; x < w_pad; x += 64) acc = fmaf(rvec[x], U[(size_t)l * w_pad + x], acc);
          acc = wave_allsum(acc);
          if (lane == 0) coef[l] = acc;
        }
        __syncthreads();
        for (int x = tid; x < w_pad; x += threads) {
          float v = rvec[x];
          for (int l = 0; l < count; ++l) v = fmaf(-coef[l], U[(size_t)l * w_pad + x], v);
          rvec[x] = v;
        }
        __syncthreads();
      }
      float acc = 0.f;
      for (int x = lane; x < w_pad; x += 64) acc = fmaf(rvec[x], rvec[x], acc);
      gain = wave_allsum(acc);  // the same bits in every wavefront
      if (!(gain > min_gain * qj * qj)) break;
      float *un = U + (size_t)count * w_pad;
      const float root = sqrtf(gain);
      for (int x = tid; x < w_pad; x += threads) un[x] = rvec[x] / root;
      __syncthreads();
      u = un;
    } else {
      gain = lambda * qj - one_minus * vj;
    }
    if (tid == 0) {
      ids_out[r * (size_t)n + count] = idj;
      gains_out[r * (size_t)n + count] = gain;
    }
    ++count;

    // ---- 3. every candidate against the step's vector ------------------------------------------------------------------------
    float uc[CPL];
#pragma unroll
    for (int x = 0; x < CPL; ++x) uc[x] = u[col0 + x];
    auto update = [&](int i, float dot) {
      if (gl == 0 && i < m_cap) {
        const float e = scale[i] * dot;
        if (rule == 0) val[i] = val[i] - e * e;
        else val[i] = count == 1 ? e : fmaxf(val[i], e);
      }
    };
    if constexpr (CPT > 0) {
#pragma unroll
      for (int t = 0; t < CPT; ++t) update(t * groups + grp, dot_cols<CPL>(frag[t], uc, G));
    } else {
      for (int i0 = 0; i0 < len; i0 += groups) {
        const int i = i0 + grp;
        const int id = i < len ? cid[i] : -1;  // a picked candidate is not read again
        float y[CPL];
        load_cols<TI, CPL>(id >= 0 ? items + (size_t)id * w : nullptr, col0, w, y);
        update(i, dot_cols<CPL>(y, uc, G));
      }
    }
  }
  for (int k = count + tid; k < n; k += threads) {
    ids_out[r * (size_t)n + k] = -1;
    gains_out[r * (size_t)n + k] = -FLT_MAX;
  }
  if (tid == 0) counts_out[r] = count;
}

struct DivCall {
  const imp_matrix *items;
  const int64_t *offsets;
  const int32_t *candidates;
  const float *quality;
  int n, rule;
  float param, min_gain;
  int32_t *indices;
  float *gains;
  int32_t *counts;
  int cpl, g, k_cap;
  bool lds_basis;
};

static int div_round_up(int v, int m) { return (v + m - 1) / m * m; }
static size_t div_fixed_lds(int m_cap, int w_pad, int k_cap) {
  return (size_t)(kDivSlotWords + 5 * (size_t)m_cap + w_pad + k_cap) * sizeof(float);
}

// device bytes of one row's share of a chunk
static size_t div_row_bytes(const DivCall &c, size_t r) {
  const size_t len = (size_t)(c.offsets[r + 1] - c.offsets[r]);
  return len * (sizeof(int32_t) + sizeof(float)) + 2 * sizeof(int64_t) + (size_t)c.n * (sizeof(int32_t) + sizeof(float)) +
         sizeof(int32_t) + (c.lds_basis ? 0 : (size_t)c.k_cap * c.g * c.cpl * sizeof(float));
}

template <typename TI, int CPL, int CPT, typename... Args>
static void div_launch(unsigned int rows, int threads, size_t lds, Args... args) {
  allow_dynamic_lds(diversify_kernel<TI, CPL, CPT>, lds);
  diversify_kernel<TI, CPL, CPT><<<rows, threads, lds, stream()>>>(args...);
}

template <typename TI, int CPL> static void div_chunk(const DivCall &c, size_t r0, size_t r1) {
  const size_t rows = r1 - r0, w = c.items->cols;
  const int64_t c0 = c.offsets[r0], nc = c.offsets[r1] - c0;
  std::vector<int64_t> h_off(rows + 1);
  int longest = 1;
  for (size_t r = 0; r <= rows; ++r) h_off[r] = c.offsets[r0 + r] - c0;
  for (size_t r = 0; r < rows; ++r) longest = std::max(longest, (int)(h_off[r + 1] - h_off[r]));
  // the launch shape, by the chunk's longest list: the smallest register form that holds it, else the streamed kernel
  constexpr int kSmall = kDivFragSmall / CPL, kFull = div_frag_full(CPL) / CPL;
  const int max_groups = kDivBlock / c.g;
  const int cpt = longest <= kSmall * max_groups ? kSmall : longest <= kFull * max_groups ? kFull : 0;
  const int threads = cpt ? std::min(kDivBlock, div_round_up((longest + cpt - 1) / cpt * c.g, 64)) : kDivBlock;
  const int w_pad = c.g * CPL;
  const DivShape shape{c.g, div_round_up(longest, threads / c.g), c.k_cap, c.lds_basis ? 1 : 0};
  const size_t lds = div_fixed_lds(shape.m_cap, w_pad, c.k_cap) + (c.lds_basis ? (size_t)c.k_cap * w_pad * sizeof(float) : 0);
  float *basis = c.lds_basis ? nullptr : ctx().div_basis.reserve(rows * (size_t)c.k_cap * w_pad);

  DeviceArray<int64_t> d_off;
  DeviceArray<int32_t> d_cand, d_ids, d_counts;
  DeviceArray<float> d_quality, d_gains;
  d_off.upload(h_off.data(), rows + 1);
  d_cand.upload(c.candidates + c0, (size_t)nc);
  d_quality.upload(c.quality + c0, (size_t)nc);
  const size_t out = rows * (size_t)c.n;
  d_ids.alloc(out);
  d_gains.alloc(out);
  d_counts.alloc(rows);
  {
    IMP_PROF("diversify");
    auto go = [&](auto cpt_tag) {
      div_launch<TI, CPL, decltype(cpt_tag)::value>((unsigned int)rows, threads, lds, c.items->as<TI>(), (int)w, shape, d_off.data(),
                                                     d_cand.data(), d_quality.data(), c.n, c.rule, c.param, c.min_gain, basis,
                                                     d_ids.data(), d_gains.data(), d_counts.data());
    };
    if (cpt == kSmall) go(std::integral_constant<int, kSmall>{});
    else if (cpt == kFull) go(std::integral_constant<int, kFull>{});
    else go(std::integral_constant<int, 0>{});
    IMP_CHECK_HIP(hipGetLastError());
  }
  IMP_CHECK_HIP(hipMemcpyAsync(c.indices + r0 * (size_t)c.n, d_ids.data(), out * sizeof(int32_t), hipMemcpyDeviceToHost, stream()));
  IMP_CHECK_HIP(hipMemcpyAsync(c.gains + r0 * (size_t)c.n, d_gains.data(), out * sizeof(float), hipMemcpyDeviceToHost, stream()));
  IMP_CHECK_HIP(hipMemcpyAsync(c.counts + r0, d_counts.data(), rows * sizeof(int32_t), hipMemcpyDeviceToHost, stream()));
  sync();  // the host vector and device arrays of the chunk die here
}

template <typename TI, int CPL> static void div_rows(const DivCall &c, size_t rows, size_t budget) {
  for (size_t r0 = 0; r0 < rows;) {  // greedy chunks of whole rows; every row fits (checked by the caller)
    size_t r1 = r0, bytes = 0;
    while (r1 < rows && r1 - r0 < (size_t)INT32_MAX) {
      const size_t b = div_row_bytes(c, r1);
      if (r1 > r0 && bytes + b > budget) break;
      bytes += b, ++r1;
    }
    div_chunk<TI, CPL>(c, r0, r1);
    r0 = r1;
  }
}

template <typename TI> static void div_dispatch(const DivCall &c, size_t rows, size_t budget) {
  if (c.cpl == 4) div_rows<TI, 4>(c, rows, budget);
  else if (c.cpl == 8) div_rows<TI, 8>(c, rows, budget);
  else div_rows<TI, 16>(c, rows, budget);
}

}  // namespace imp

using namespace imp;

extern "C" int imp_knn_diversify(imp_knn *knn, const imp_matrix *items, int64_t n_rows, const int64_t *offsets,
                                 const int32_t *candidates, const float *quality, int n, int rule, float param, float min_gain,
                                 int32_t *indices, float *gains, int32_t *counts) {
  return guarded([&] {
    const size_t w = items->cols;
    if (w < 1 || w > (size_t)kDivMaxWidth)
      throw std::invalid_argument("diversify: the item factors need 1 .. " + std::to_string(kDivMaxWidth) + " columns, got " + std::to_string(w));
    if (items->itemsize != 4 && items->itemsize != 2) throw std::invalid_argument("diversify: items must be float32 or float16");
    if (items->rows > (size_t)INT32_MAX) throw std::invalid_argument("diversify: too many items");
    if (n < 1) throw std::invalid_argument("diversify: n must be >= 1");
    if (rule != 0 && rule != 1) throw std::invalid_argument("diversify: rule must be 0 (DPP) or 1 (MMR)");
    if (rule == 1 && !(param >= 0.f && param <= 1.f)) throw std::invalid_argument("diversify: MMR's lambda must lie in [0, 1]");
    if (rule == 0 && !(min_gain >= 0.f && min_gain < 1.f)) throw std::invalid_argument("diversify: min_gain must lie in [0, 1)");
    if (n_rows < 0 || n_rows > (int64_t)INT32_MAX) throw std::invalid_argument("diversify: rows must lie in 0 .. 2^31 - 1");
    const size_t rows = (size_t)n_rows;
    if (rows == 0) return;
    if (offsets[0] != 0) throw std::invalid_argument("diversify: offsets must start at 0");
    int64_t longest = 0;
    for (size_t r = 0; r < rows; ++r) {
      const int64_t len = offsets[r + 1] - offsets[r];
      if (len < 0) throw std::invalid_argument("diversify: offsets decrease at row " + std::to_string(r));
      if (len > kDivMaxList)
        throw std::invalid_argument("diversify: the list of row " + std::to_string(r) + " holds " + std::to_string(len) +
                                    " candidates, at most " + std::to_string(kDivMaxList) + " are supported");
      longest = std::max(longest, len);
    }
    const int64_t total = offsets[rows];
    for (int64_t e = 0; e < total; ++e) {
      if (candidates[e] < 0 || (size_t)candidates[e] >= items->rows)
        throw std::invalid_argument("diversify: candidate id " + std::to_string(candidates[e]) + " (position " + std::to_string(e) +
                                    ") is outside the item factors (" + std::to_string(items->rows) + " rows)");
      if (!std::isfinite(quality[e]) || (rule == 0 && quality[e] < 0.f))
        throw std::invalid_argument("diversify: the quality at position " + std::to_string(e) +
                                    (rule == 0 ? " is not finite and >= 0" : " is not finite"));
    }
    DivCall c{items, offsets, candidates, quality, n, rule, param, min_gain, indices, gains, counts, 0, 0, 0, true};
    c.cpl = w <= 32 ? 4 : w <= 512 ? 8 : 16;
    c.g = 1;
    while ((size_t)c.g * c.cpl < w) c.g <<= 1;
    c.k_cap = rule == 0 ? (int)std::min<int64_t>({(int64_t)n, (int64_t)w, std::max<int64_t>(longest, 1)}) : 0;
    const int w_pad = c.g * c.cpl;
    c.lds_basis = div_fixed_lds(div_round_up((int)std::max<int64_t>(longest, 1), kDivBlock), w_pad, c.k_cap) +
                      (size_t)c.k_cap * w_pad * sizeof(float) <= kDivLdsLimit;
    const size_t budget = knn_temp_budget(knn);
    for (size_t r = 0; r < rows; ++r) {
      const size_t need = div_row_bytes(c, r);
      if (need > budget)
        throw std::invalid_argument("diversify: row " + std::to_string(r) + " alone needs " + std::to_string(need) +
                                    " bytes of temporaries, max_temp_memory is " + std::to_string(budget));
    }
    if (items->itemsize == 2) div_dispatch<__half>(c, rows, budget);
    else div_dispatch<float>(c, rows, budget);
  });
}
