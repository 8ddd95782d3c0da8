// K27: GRU4Rec -- session-based next-item recommendation (Hidasi, Karatzoglou, Baltrunas, Tikk, ICLR 2016; Hidasi and
// Karatzoglou, "Recurrent Neural Networks with Top-k Gains", CIKM 2018), one GRU layer on one-hot item input, trained session-
// parallel with in-batch and shared extra negatives: imp_gru_gradients, imp_gru_steps, imp_gru_encode, imp_host_gru_fold_plan.
//
// No reference counterpart.  All parameters are float32.  H = hidden width, a multiple of 32 in 32 .. 512.
//   W_x [items x 3H], read by row; columns 0 .. H - 1 reset gate r, H .. 2H - 1 update gate z, 2H .. 3H - 1 candidate c;
//   W_h [H x 3H], the same column order;  b [1 x 3H];  W_out [items x (H + 1)], the output bias its last column.
// A step works on B slots (a multiple of 64 in 64 .. 1024), each walking one session.  HOST arrays of a step: inputs[r] (an item
// id, -1: the slot is idle), targets[r] (the item that follows), reset[r] (1: the slot starts a session here), negatives[n],
// n < N, N a multiple of 64 in 0 .. 4096, shared by all rows.  Device state: h [B x H], read and written.
//   forward, active slot r with input i:  h0 = 0 when reset[r], else h[r];
//     a_rz = W_x[i, :2H] + b[:2H] + h0 W_h[:, :2H];  r = sigmoid(a_r), z = sigmoid(a_z);
//     a_c = W_x[i, 2H:] + b[2H:] + (r o h0) W_h[:, 2H:];  c = tanh(a_c);  h1 = (1 - z) o h0 + z o c, written back to h[r].
//     An idle slot keeps its row of h and contributes nothing anywhere.
//   scores s_rj = W_out[item_j, :H] . h1_r + W_out[item_j, H] over S = B + N columns: column j < B is targets[j] (the column of
//     an idle slot takes part in no row), column B + n is negatives[n].  Column j != r is masked for row r when item_j =
//     targets[r].  s_rr itself is one dot product per row, the same value wherever it is used.
//   losses, A = the number of active slots (A = 0: loss 0, no update):
//     "cross-entropy": L = (1 / A) sum_r (lse_r - s_rr), lse over the unmasked columns of row r, its own included;
//     "bpr-max": over the unmasked negatives j != r, p_rj their softmax, P_r = sum_j p_rj sigmoid(s_rr - s_rj), R_r = sum_j p_rj
//       s_rj^2:  L = (1 / A) sum_r (-log(P_r + 1e-24) + bpreg R_r); a row without an unmasked negative contributes 0.
//     Every exponential is of a score minus a running maximum.
//   backward, truncated at the step (h0 is a constant):  g = dL/ds;  dcol_j = sum_r g_rj [h1_r | 1];  dh1_r = sum_j g_rj
//     W_out[item_j, :H];  dz = dh1 o (c - h0) o z (1 - z);  dc = dh1 o z o (1 - c^2);  dr = (dc W_h[:, 2H:]^T) o h0 o r (1 - r);
//     da = [dr | dz | dc];  db = sum_r da_r;  dW_x[inputs[r]] += da_r;  dW_h[:, :2H] = h0^T [dr | dz];  dW_h[:, 2H:] = (r o h0)^T dc.
//   update (imp_gru_steps), Adagrad on the step's whole gradient G: acc += G^2; p -= lr G / sqrt(acc + 1e-6).  An item row that
//     occurs several times in a step (as an input; among the S columns) receives ONE update from the SUM of its occurrences,
//     taken in ascending slot / column order.  Rows that do not occur are neither read nor written.
//
// Kernels (256 threads = 4 wavefronts).  Every dense product is a 64 x 64 output block per workgroup on
// v_mfma_f32_32x32x2_f32, exact fp32, one chain per element in ascending inner index, both operands staged through LDS panels
// in chunks of 32 k and loaded one chunk ahead (the block product of mult_vae.hip, with the operand loads as functors so that a
// panel can be a gather: Rows, Cols, GatherK below).  The gates are two phases split over column blocks -- a workgroup that
// owned 64 slots and every column would leave B / 64 <= 16 workgroups on 256 compute units, and at H = 512 its resident h0
// and r o h0 alone are 256 KB; the second phase needs r over all columns of a slot, which the launch boundary supplies.
//   gates_rz  grid (rows / 64) x (H / 32): 64 slots x (32 columns of r and the SAME 32 of z); A = the rows of h (absent where the
//             slot is fresh or idle), B = W_h.  Epilogue: the gathered row of W_x, bias, sigmoid; writes r, z, h0, r o h0.
//   gates_c   grid (rows / 64) x (H / 64): (r o h0) W_h[:, 2H:]; epilogue: W_x gather, bias, tanh, the blend; writes c and h1.
//   scores<1> grid (B / 64) x (S / 64): one 64 x 64 score tile, A = h1, B = the tile's 64 gathered rows of W_out; the tile goes
//             to an LDS plane, four threads per row reduce it to (max, sum exp, and for bpr-max the three weighted sums) of the
//             tile, written to stats[plane][tile][row].  The scores are never stored.
//   merge     one workgroup: per row the tiles' statistics folded in ascending tile order, the row's loss, and the step's
//             loss summed in a fixed order.
//   scores<2> the same tile again from the same operands in the same order, turned into g and written to G [B x S].
//   back_out  two products over G in one launch: dh1 = G W_out[item] (K = S, the B operand gathered by k) with dz, dc as its
//             epilogue, and dcol = G^T h1 (K = B, ascending slot order); the bias column of dcol as column sums of G.
//   back_r    dr = (dc W_h[:, 2H:]^T) o h0 o r (1 - r), W_h read transposed from the same LDS panel layout.
//   back_w    dW_h = [h0^T (dr | dz) | (r o h0)^T dc] (K = B) and db = column sums of da, rows ascending.
//   update    one wavefront per touched row of W_x and of W_out: sums the row's occurrences of da / dcol in the order of the
//             host's fold plan and applies Adagrad; further workgroups apply it densely to W_h and b.  No atomics.
// Launches of a step: 9 (8 for imp_gru_gradients).  The phases are ordered by the launch boundaries of one stream; no workgroup
// waits for another.  G (B x S words) is stored between scores<2> and back_out: the two products that consume it reduce over
// different indices, and storing it keeps each a single ascending chain without partial planes.
//
// LDS: two operand panels of 2112 words ([64][k] with leading dimension 33, or [k][64] with leading dimension 65, as in
// mult_vae.hip), and for gates_rz and scores a 64 x 65 plane: 33 536 bytes, scores 36 096 with its id and row words.
//
// Fold plan (host only, fold_plan below; imp_host_gru_fold_plan exposes it): the ids of a step that are >= 0, stably sorted; the
// unique ids ascending, and for each its positions ascending.  Everything the three calls return or update is bit-
// reproducible on one device.  Every address is bounded: ids are checked on the host before anything is queued, block rows
// and columns beyond a matrix are loaded as 0 and never stored.  Whatever a later kernel reads is written with agent-scope
// stores.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "common.h"

namespace imp {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTile = 64;
constexpr int kKc = 32;                // k per staged chunk
constexpr int kLdK = kKc + 1;          // a panel stored [64][k]
constexpr int kLdT = kTile + 1;        // a panel stored [k][64], and the score plane
constexpr int kPanel = kTile * kLdK;   // 2112 words >= 32 x 65
constexpr int kPlanes = 5;             // max, sum exp, and the sigmoid-, square- and slope-weighted sums of bpr-max

__device__ __forceinline__ void store_through(float *p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// row of element e of a lane's 32 x 32 accumulator; its column is lane & 31
__device__ __forceinline__ int tile_row(int e, int lane) { return (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5); }
__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---- operand panels: 64 rows (A) or columns (B) of a block, 32 k at a time --------------------------------------------------
// k is the COLUMN index of the stored matrix; block element i is the row that starts at offset off(i), or absent (< 0)
struct Rows {
  static constexpr bool kmajor = false;
  const float *__restrict__ p;
  long off[8];  // of this thread's rows (threadIdx.x >> 5) + 8 j
  template <typename F> __device__ __forceinline__ Rows(const float *p_, F offset_of) : p(p_) {
#pragma unroll
    for (int j = 0; j < 8; ++j) off[j] = offset_of((int)(threadIdx.x >> 5) + 8 * j);
  }
  __device__ __forceinline__ void load(int k0, float (&r)[8]) const {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = off[j] >= 0 ? p[off[j] + k0 + (threadIdx.x & 31)] : 0.f;
  }
};
// k is the ROW index of the stored matrix (leading dimension ld); this thread's block element is column `at` (< 0: absent;
// == one: a column of 1.0 that is not stored)
struct Cols {
  static constexpr bool kmajor = true;
  const float *__restrict__ p;
  int ld, at, one;
  __device__ __forceinline__ void load(int k0, float (&r)[8]) const {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = at < 0 ? 0.f : at == one ? 1.0f : p[(size_t)(k0 + (threadIdx.x >> 6) + 4 * j) * ld + at];
  }
};
// as Cols, but row k of the operand is row ids[k] of the stored matrix (absent where ids[k] < 0)
struct GatherK {
  static constexpr bool kmajor = true;
  const float *__restrict__ p;
  const int32_t *__restrict__ ids;
  int ld, at;
  __device__ __forceinline__ void load(int k0, float (&r)[8]) const {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int id = ids[k0 + (threadIdx.x >> 6) + 4 * j];
      r[j] = at >= 0 && id >= 0 ? p[(size_t)id * ld + at] : 0.f;
    }
  }
};
template <bool KMAJOR> __device__ __forceinline__ void panel_store(float *S, const float (&r)[8]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (KMAJOR) S[((tid >> 6) + 4 * j) * kLdT + (tid & 63)] = r[j];
    else S[((tid >> 5) + 8 * j) * kLdK + (tid & 31)] = r[j];
  }
}
template <bool KMAJOR> __device__ __forceinline__ float panel_read(const float *S, int i, int k) {
  return KMAJOR ? S[k * kLdT + i] : S[i * kLdK + k];
}

// This wavefront's 32 x 32 block of A B over K (a multiple of 32): rows 32 (wave & 1) .., columns 32 (wave >> 1) .. of the
// workgroup's 64 x 64 block.  All 256 threads call it; As and Bs are free again when it returns.
template <typename LA, typename LB> __device__ __forceinline__ f32x16 block_product(const LA &A, const LB &Bp, int K, float *As, float *Bs) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, lk = lane >> 5;
  const int mw = 32 * (wave & 1) + l31, nw = 32 * (wave >> 1) + l31;
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  float ra[8], rb[8];
  A.load(0, ra);
  Bp.load(0, rb);
  for (int k0 = 0; k0 < K; k0 += kKc) {
    panel_store<LA::kmajor>(As, ra);
    panel_store<LB::kmajor>(Bs, rb);
    __syncthreads();
    if (k0 + kKc < K) {
      A.load(k0 + kKc, ra);
      Bp.load(k0 + kKc, rb);
    }
#pragma unroll
    for (int ks = 0; ks < kKc / 2; ++ks)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(panel_read<LA::kmajor>(As, mw, 2 * ks + lk), panel_read<LB::kmajor>(Bs, nw, 2 * ks + lk), acc, 0, 0, 0);
    __syncthreads();
  }
  return acc;
}

// ---- the gates ----------------------------------------------------------------------------------------------------------------
struct Gates {
  const float *h;                      // rows x H, the state before the step (h1 may be the same memory)
  const int32_t *__restrict__ inputs;  // [rows], -1: idle
  const int32_t *__restrict__ reset;   // [rows], or NULL with reset_all
  int reset_all, rows, H;
  const float *__restrict__ W_x;
  const float *__restrict__ W_h;
  const float *__restrict__ b;
  float *r, *z, *h0, *rh, *c;  // rows x H; r and c may be NULL (forward only)
  float *h1;                   // rows x H: may be h itself
};

__global__ __launch_bounds__(256) void gru_gates_rz_kernel(Gates a) {
  __shared__ float As[kPanel], Bs[kPanel], Cs[kTile * kLdT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31;
  const int H = a.H, rows = a.rows, blocks = H / 32;
  const int m0 = (int)(blockIdx.x / blocks) * kTile, cb = blockIdx.x % blocks;
  auto carried = [&](int row) { return row < rows && a.inputs[row] >= 0 && !(a.reset_all || (a.reset && a.reset[row])); };
  const Rows A(a.h, [&](int i) { return carried(m0 + i) ? (long)(m0 + i) * H : -1L; });
  const int i64 = tid & 63;
  const Cols W{a.W_h, 3 * H, i64 < 32 ? 32 * cb + i64 : H + 32 * cb + i64 - 32, -2};
  const f32x16 acc = block_product(A, W, H, As, Bs);
#pragma unroll
  for (int e = 0; e < 16; ++e) Cs[(32 * (wave & 1) + tile_row(e, lane)) * kLdT + 32 * (wave >> 1) + l31] = acc[e];
  __syncthreads();
  const int col = 32 * cb + l31;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int row = (tid >> 5) + 8 * i, s = m0 + row;
    if (s >= rows) continue;
    const int item = a.inputs[s];
    float r = 0.f, z = 0.f, h0 = 0.f;
    if (item >= 0) {
      const float *wx = a.W_x + (size_t)item * 3 * H;
      r = sigmoidf((wx[col] + a.b[col]) + Cs[row * kLdT + l31]);
      z = sigmoidf((wx[H + col] + a.b[H + col]) + Cs[row * kLdT + 32 + l31]);
      h0 = carried(s) ? a.h[(size_t)s * H + col] : 0.f;
    }
    const size_t at = (size_t)s * H + col;
    if (a.r) store_through(a.r + at, r);
    store_through(a.z + at, z);
    store_through(a.h0 + at, h0);
    store_through(a.rh + at, r * h0);
  }
}

__global__ __launch_bounds__(256) void gru_gates_c_kernel(Gates a) {
  __shared__ float As[kPanel], Bs[kPanel];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31;
  const int H = a.H, rows = a.rows, blocks = (H + kTile - 1) / kTile;
  const int m0 = (int)(blockIdx.x / blocks) * kTile, n0 = (int)(blockIdx.x % blocks) * kTile;
  const Rows A(a.rh, [&](int i) { return m0 + i < rows ? (long)(m0 + i) * H : -1L; });
  const int i64 = tid & 63;
  const Cols W{a.W_h, 3 * H, n0 + i64 < H ? 2 * H + n0 + i64 : -1, -2};
  const f32x16 acc = block_product(A, W, H, As, Bs);
  const int col = n0 + 32 * (wave >> 1) + l31;
  if (col >= H) return;
  const float bias = a.b[2 * H + col];
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int s = m0 + 32 * (wave & 1) + tile_row(e, lane);
    if (s >= rows) continue;
    const size_t at = (size_t)s * H + col;
    const int item = a.inputs[s];
    if (item < 0) {  // idle: the row of h stays
      if (a.c) store_through(a.c + at, 0.f);
      if (a.h1 != a.h) store_through(a.h1 + at, a.h[at]);
      continue;
    }
    const float c = tanhf((a.W_x[(size_t)item * 3 * H + 2 * H + col] + bias) + acc[e]);
    const float z = a.z[at], h0 = a.h0[at];
    if (a.c) store_through(a.c + at, c);
    store_through(a.h1 + at, (1.0f - z) * h0 + z * c);
  }
}

// ---- scores -------------------------------------------------------------------------------------------------------------------
struct Scores {
  const float *__restrict__ h1;      // B x H
  const float *__restrict__ W_out;   // items x (H + 1)
  const int32_t *__restrict__ cols;  // [S] item of column j, -1: takes part in no row
  const int32_t *__restrict__ rows;  // [B] target of slot r, -1: idle
  int B, S, H;
  float inv_active, bpreg;
  float *stats;     // [kPlanes][S / 64][B]
  float *diag;      // [B] s_rr
  float *rowstat;   // [B][8]: M, E, P, R, D, s_rr, live
  float *G;         // B x S
  float *loss;      // one word
};

// The score tile of row block m0 and column tile j0 in Cs; ids, targets and s_rr of the tile in the LDS words.
__device__ __forceinline__ void score_tile(const Scores &a, int m0, int j0, float *As, float *Bs, float *Cs, int *cid, int *tgt, float *srr) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, H = a.H;
  if (tid < kTile) cid[tid] = a.cols[j0 + tid], tgt[tid] = a.rows[m0 + tid];
  __syncthreads();
  {  // s_rr: four threads per row, k = part, part + 4, ... ascending, then the four by an xor butterfly
    const int row = tid >> 2, part = tid & 3, t = tgt[row];
    float s = 0.f;
    if (t >= 0) {
      const float *w = a.W_out + (size_t)t * (H + 1), *h = a.h1 + (size_t)(m0 + row) * H;
      for (int k = part; k < H; k += 4) s += h[k] * w[k];
    }
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    if (part == 0) srr[row] = t >= 0 ? s + a.W_out[(size_t)t * (H + 1) + H] : 0.f;
  }
  const Rows A(a.h1, [&](int i) { return (long)(m0 + i) * H; });
  const Rows W(a.W_out, [&](int i) { return cid[i] >= 0 ? (long)cid[i] * (H + 1) : -1L; });
  const f32x16 acc = block_product(A, W, H, As, Bs);
  const int n = 32 * (wave >> 1) + l31;
  const float bias = cid[n] >= 0 ? a.W_out[(size_t)cid[n] * (H + 1) + H] : 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) Cs[(32 * (wave & 1) + tile_row(e, lane)) * kLdT + n] = acc[e] + bias;
  __syncthreads();
}

// 0: masked;  1: an unmasked negative;  2: the row's own column
__device__ __forceinline__ int column_kind(int r, int j, int item, int target) {
  if (item < 0 || target < 0) return 0;
  if (j == r) return 2;
  return item != target;
}

template <int PASS, bool BPR> __global__ __launch_bounds__(256) void gru_scores_kernel(Scores a) {
  __shared__ float As[kPanel], Bs[kPanel], Cs[kTile * kLdT], srr[kTile], rs[kTile * 8];
  __shared__ int cid[kTile], tgt[kTile];
  const int tid = threadIdx.x, tiles = a.S / kTile;
  const int m0 = (int)(blockIdx.x / tiles) * kTile, tile = blockIdx.x % tiles, j0 = tile * kTile;
  if (PASS == 2)
    for (int i = tid; i < kTile * 8; i += 256) rs[i] = a.rowstat[(size_t)m0 * 8 + i];
  score_tile(a, m0, j0, As, Bs, Cs, cid, tgt, srr);
  if (PASS == 1) {
    const int row = tid >> 2, part = tid & 3, r = m0 + row;
    const float own = srr[row];
    float m = -INFINITY;
    for (int q = 0; q < 16; ++q) {
      const int jj = part + 4 * q, kind = column_kind(r, j0 + jj, cid[jj], tgt[row]);
      if (kind == 1) m = fmaxf(m, Cs[row * kLdT + jj]);
      if (kind == 2 && !BPR) m = fmaxf(m, own);
    }
    m = fmaxf(m, __shfl_xor(m, 1));
    m = fmaxf(m, __shfl_xor(m, 2));
    float sum[4] = {0.f, 0.f, 0.f, 0.f};
    for (int q = 0; q < 16; ++q) {
      const int jj = part + 4 * q, kind = column_kind(r, j0 + jj, cid[jj], tgt[row]);
      if (kind == 0 || (kind == 2 && BPR)) continue;
      const float s = kind == 2 ? own : Cs[row * kLdT + jj], w = expf(s - m);
      sum[0] += w;
      if (BPR) {
        const float sg = sigmoidf(own - s);
        sum[1] += w * sg, sum[2] += w * (s * s), sum[3] += w * (sg * (1.0f - sg));
      }
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) sum[p] += __shfl_xor(sum[p], 1), sum[p] += __shfl_xor(sum[p], 2);
    if (part == 0) {
      const size_t plane = (size_t)tiles * a.B, at = (size_t)tile * a.B + r;
      store_through(a.stats + at, m);
#pragma unroll
      for (int p = 0; p < 4; ++p)
        if (p == 0 || BPR) store_through(a.stats + (p + 1) * plane + at, sum[p]);
      if (tile == 0) store_through(a.diag + r, own);
    }
    return;
  }
  for (int idx = tid; idx < kTile * kTile; idx += 256) {
    const int row = idx >> 6, jj = idx & 63, r = m0 + row;
    const float *st = rs + row * 8;  // M, E, P, R, D, s_rr, live
    const int kind = st[6] != 0.f ? column_kind(r, j0 + jj, cid[jj], tgt[row]) : 0;
    float g = 0.f;
    if (kind) {
      const float own = st[5], s = kind == 2 ? own : Cs[row * kLdT + jj];
      if (!BPR) {
        g = expf(s - st[0]) / st[1] - (kind == 2 ? 1.0f : 0.f);
      } else if (kind == 2) {
        g = -st[4] / (st[2] + 1e-24f);
      } else {
        const float p = expf(s - st[0]) / st[1], sg = sigmoidf(own - s);
        g = a.bpreg * (p * ((s * s + 2.0f * s) - st[3])) - (p * (sg * sg - st[2])) / (st[2] + 1e-24f);
      }
      g *= a.inv_active;
    }
    store_through(a.G + (size_t)r * a.S + j0 + jj, g);
  }
}

// one workgroup: folds the tiles' statistics per row, in ascending tile order, and sums the rows' losses in a fixed order
template <bool BPR> __global__ __launch_bounds__(256) void gru_merge_kernel(Scores a) {
  __shared__ float part[256];
  const int tid = threadIdx.x, tiles = a.S / kTile;
  const size_t plane = (size_t)tiles * a.B;
  float total = 0.f;
  for (int r = tid; r < a.B; r += 256) {
    float M = -INFINITY;
    for (int t = 0; t < tiles; ++t) M = fmaxf(M, a.stats[(size_t)t * a.B + r]);
    float sum[4] = {0.f, 0.f, 0.f, 0.f};
    const bool live = a.rows[r] >= 0 && M > -INFINITY;
    if (live)
      for (int t = 0; t < tiles; ++t) {
        const size_t at = (size_t)t * a.B + r;
        const float m = a.stats[at];
        if (!(m > -INFINITY)) continue;
        const float w = expf(m - M);
#pragma unroll
        for (int p = 0; p < 4; ++p)
          if (p == 0 || BPR) sum[p] += a.stats[(p + 1) * plane + at] * w;
      }
    const float own = a.diag[r], E = sum[0], P = live ? sum[1] / E : 0.f, R = live ? sum[2] / E : 0.f, D = live ? sum[3] / E : 0.f;
    float *st = a.rowstat + (size_t)r * 8;
    store_through(st + 0, live ? M : 0.f), store_through(st + 1, live ? E : 1.0f), store_through(st + 2, P), store_through(st + 3, R);
    store_through(st + 4, D), store_through(st + 5, own), store_through(st + 6, live ? 1.0f : 0.f), store_through(st + 7, 0.f);
    if (live) total += BPR ? a.bpreg * R - logf(P + 1e-24f) : (M + logf(E)) - own;
  }
  part[tid] = total;
  __syncthreads();
  for (int half = 128; half; half >>= 1) {
    if (tid < half) part[tid] += part[tid + half];
    __syncthreads();
  }
  if (tid == 0) store_through(a.loss, part[0] * a.inv_active);
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
struct Back {
  int B, S, H;
  const float *__restrict__ G;         // B x S
  const int32_t *__restrict__ cols;    // [S]
  const float *__restrict__ W_out;
  const float *__restrict__ W_h;
  const float *__restrict__ h1;
  const float *__restrict__ r;
  const float *__restrict__ z;
  const float *__restrict__ c;
  const float *__restrict__ h0;
  const float *__restrict__ rh;
  float *dh1, *da, *dcol, *dW_h, *db;  // B x H, B x 3H, S x (H + 1), H x 3H, 3H
};

// dh1 = G W_out[item] with dz and dc as its epilogue;  dcol[:, :H] = G^T h1;  dcol[:, H] = the column sums of G
__global__ __launch_bounds__(256) void gru_back_out_kernel(Back a) {
  __shared__ float As[kPanel], Bs[kPanel];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, i64 = tid & 63;
  const int B = a.B, S = a.S, H = a.H, hb = (H + kTile - 1) / kTile;
  const int row_wise = (B / kTile) * hb, col_wise = (S / kTile) * hb;
  int id = blockIdx.x;
  if (id < row_wise) {
    const int m0 = (id / hb) * kTile, n0 = (id % hb) * kTile;
    const Rows A(a.G, [&](int i) { return (long)(m0 + i) * S; });
    const GatherK W{a.W_out, a.cols, H + 1, n0 + i64 < H ? n0 + i64 : -1};
    const f32x16 acc = block_product(A, W, S, As, Bs);
    const int col = n0 + 32 * (wave >> 1) + l31;
    if (col >= H) return;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int r = m0 + 32 * (wave & 1) + tile_row(e, lane);
      const size_t at = (size_t)r * H + col;
      const float z = a.z[at], c = a.c[at], h0 = a.h0[at], d = acc[e];
      store_through(a.dh1 + at, d);
      store_through(a.da + (size_t)r * 3 * H + H + col, (d * (c - h0)) * (z * (1.0f - z)));
      store_through(a.da + (size_t)r * 3 * H + 2 * H + col, (d * z) * (1.0f - c * c));
    }
    return;
  }
  id -= row_wise;
  if (id < col_wise) {
    const int j0 = (id / hb) * kTile, n0 = (id % hb) * kTile;
    const Cols A{a.G, S, j0 + i64, -2}, X{a.h1, H, n0 + i64 < H ? n0 + i64 : -1, -2};
    const f32x16 acc = block_product(A, X, B, As, Bs);
    const int col = n0 + 32 * (wave >> 1) + l31;
    if (col >= H) return;
#pragma unroll
    for (int e = 0; e < 16; ++e) store_through(a.dcol + (size_t)(j0 + 32 * (wave & 1) + tile_row(e, lane)) * (H + 1) + col, acc[e]);
    return;
  }
  id -= col_wise;
  const int j = id * 256 + tid;
  if (j >= S) return;
  float s = 0.f;
  for (int r = 0; r < B; ++r) s += a.G[(size_t)r * S + j];
  store_through(a.dcol + (size_t)j * (H + 1) + H, s);
}

__global__ __launch_bounds__(256) void gru_back_r_kernel(Back a) {
  __shared__ float As[kPanel], Bs[kPanel];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31;
  const int H = a.H, hb = (H + kTile - 1) / kTile;
  const int m0 = (int)(blockIdx.x / hb) * kTile, n0 = (int)(blockIdx.x % hb) * kTile;
  const Rows A(a.da, [&](int i) { return (long)(m0 + i) * 3 * H + 2 * H; });
  const Rows W(a.W_h, [&](int i) { return n0 + i < H ? (long)(n0 + i) * 3 * H + 2 * H : -1L; });
  const f32x16 acc = block_product(A, W, H, As, Bs);
  const int col = n0 + 32 * (wave >> 1) + l31;
  if (col >= H) return;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int r = m0 + 32 * (wave & 1) + tile_row(e, lane);
    const size_t at = (size_t)r * H + col;
    const float g = a.r[at];
    store_through(a.da + (size_t)r * 3 * H + col, (acc[e] * a.h0[at]) * (g * (1.0f - g)));
  }
}

__global__ __launch_bounds__(256) void gru_back_w_kernel(Back a) {
  __shared__ float As[kPanel], Bs[kPanel];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, i64 = tid & 63;
  const int B = a.B, H = a.H, hb = (H + kTile - 1) / kTile, cb = (3 * H + kTile - 1) / kTile;
  int id = blockIdx.x;
  if (id < hb * cb) {
    const int m0 = (id / cb) * kTile, n0 = (id % cb) * kTile;  // 2H is a multiple of 64: a column block lies on one side of it
    const Cols A{n0 < 2 * H ? a.h0 : a.rh, H, m0 + i64 < H ? m0 + i64 : -1, -2}, D{a.da, 3 * H, n0 + i64 < 3 * H ? n0 + i64 : -1, -2};
    const f32x16 acc = block_product(A, D, B, As, Bs);
    const int col = n0 + 32 * (wave >> 1) + l31;
    if (col >= 3 * H) return;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int m = m0 + 32 * (wave & 1) + tile_row(e, lane);
      if (m < H) store_through(a.dW_h + (size_t)m * 3 * H + col, acc[e]);
    }
    return;
  }
  id -= hb * cb;
  const int col = id * 256 + tid;
  if (col >= 3 * H) return;
  float s = 0.f;
  for (int r = 0; r < B; ++r) s += a.da[(size_t)r * 3 * H + col];
  store_through(a.db + col, s);
}

// ---- fold and Adagrad -----------------------------------------------------------------------------------------------------------
struct FoldSide {
  float *param, *accum;             // rows x width
  const float *__restrict__ grad;   // per occurrence: [position] x width
  const int32_t *__restrict__ ids;  // [n] the touched rows, ascending
  const int32_t *__restrict__ start;  // [n + 1]
  const int32_t *__restrict__ occ;    // positions, ascending within a row
  int n, width;
};
struct Update {
  FoldSide x, o;
  float *W_h, *acc_W_h, *b, *acc_b;
  const float *__restrict__ dW_h;
  const float *__restrict__ db;
  int n_wh, n_b;
  float lr;
};

__device__ __forceinline__ void adagrad(float *p, float *acc, float g, float lr) {
  const float v = *acc + g * g;
  store_through(acc, v);
  store_through(p, *p - (lr * g) / sqrtf(v + 1e-6f));
}

__global__ __launch_bounds__(256) void gru_update_kernel(Update a) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int row_groups = (a.x.n + a.o.n + 3) / 4;
  if ((int)blockIdx.x < row_groups) {
    int u = (int)blockIdx.x * 4 + (tid >> 6);
    if (u >= a.x.n + a.o.n) return;
    const FoldSide &s = u < a.x.n ? a.x : a.o;
    if (u >= a.x.n) u -= a.x.n;
    const int lo = s.start[u], hi = s.start[u + 1];
    const size_t at = (size_t)s.ids[u] * s.width;
    for (int col = lane; col < s.width; col += 64) {
      float g = 0.f;
      for (int e = lo; e < hi; ++e) g += s.grad[(size_t)s.occ[e] * s.width + col];
      adagrad(s.param + at + col, s.accum + at + col, g, a.lr);
    }
    return;
  }
  const int i = ((int)blockIdx.x - row_groups) * 256 + tid;
  if (i < a.n_wh) adagrad(a.W_h + i, a.acc_W_h + i, a.dW_h[i], a.lr);
  else if (i < a.n_wh + a.n_b) adagrad(a.b + i - a.n_wh, a.acc_b + i - a.n_wh, a.db[i - a.n_wh], a.lr);
}

// out[order[s]] = [h[s] | 1]
__global__ __launch_bounds__(256) void gru_emit_kernel(const float *__restrict__ h, const int32_t *__restrict__ order, int n, int H, float *out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)n * (H + 1)) return;
  const int s = (int)(i / (H + 1)), col = (int)(i % (H + 1));
  store_through(out + (size_t)order[s] * (H + 1) + col, col < H ? h[(size_t)s * H + col] : 1.0f);
}
__global__ __launch_bounds__(256) void gru_zero_kernel(float *p, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) store_through(p + i, 0.f);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
size_t round64(size_t n) { return (n + 63) / 64 * 64; }

// The fold plan of n ids (those < 0 take no part): the unique ids ascending, start[u] .. start[u + 1] the slice of occ that
// holds the positions of unique[u], ascending.
struct FoldPlan {
  std::vector<int32_t> unique, start, occ;
};
FoldPlan fold_plan(const int32_t *ids, int64_t n) {
  FoldPlan p;
  for (int64_t i = 0; i < n; ++i)
    if (ids[i] >= 0) p.occ.push_back((int32_t)i);
  std::stable_sort(p.occ.begin(), p.occ.end(), [&](int32_t x, int32_t y) { return ids[x] < ids[y]; });
  for (size_t e = 0; e < p.occ.size(); ++e)
    if (e == 0 || ids[p.occ[e]] != ids[p.occ[e - 1]]) p.unique.push_back(ids[p.occ[e]]), p.start.push_back((int32_t)e);
  p.start.push_back((int32_t)p.occ.size());
  return p;
}

struct Shape {
  int items, H, B, N, S;
  bool bpr;
};

int hidden_of(const std::string &w, const imp_matrix *W_x, const imp_matrix *W_h, const imp_matrix *b, const imp_matrix *W_out) {
  for (const imp_matrix *m : {W_x, W_h, b, W_out})
    if (m && m->itemsize != 4) throw std::invalid_argument(w + ": parameters must be float32");
  const size_t H = W_h->rows;
  if (H < 32 || H > 512 || H % 32) throw std::invalid_argument(w + ": hidden must be a multiple of 32 in 32 .. 512");
  if (W_h->cols != 3 * H) throw std::invalid_argument(w + ": W_h must be hidden x (3 hidden)");
  if (W_x->cols != 3 * H || W_x->rows < 1 || W_x->rows > (size_t)INT32_MAX) throw std::invalid_argument(w + ": W_x must be items x (3 hidden)");
  if (b->rows != 1 || b->cols != 3 * H) throw std::invalid_argument(w + ": b must be 1 x (3 hidden)");
  if (W_out && (W_out->rows != W_x->rows || W_out->cols != H + 1)) throw std::invalid_argument(w + ": W_out must be items x (hidden + 1)");
  return (int)H;
}

Shape shape_of(const std::string &w, const imp_matrix *W_x, const imp_matrix *W_h, const imp_matrix *b, const imp_matrix *W_out,
               const imp_matrix *h, int64_t B, int64_t N, const char *loss, float bpreg) {
  Shape s{};
  s.H = hidden_of(w, W_x, W_h, b, W_out);
  s.items = (int)W_x->rows;
  if (B < 64 || B > 1024 || B % 64) throw std::invalid_argument(w + ": batch_size must be a multiple of 64 in 64 .. 1024");
  if (N < 0 || N > 4096 || N % 64) throw std::invalid_argument(w + ": the number of negatives must be a multiple of 64 in 0 .. 4096");
  if (!h || h->itemsize != 4 || h->rows != (size_t)B || h->cols != (size_t)s.H) throw std::invalid_argument(w + ": h must be float32, batch_size x hidden");
  if (!loss || (strcmp(loss, "cross-entropy") && strcmp(loss, "bpr-max"))) throw std::invalid_argument(w + ": loss must be \"cross-entropy\" or \"bpr-max\"");
  s.bpr = !strcmp(loss, "bpr-max");
  if (!(bpreg >= 0.f)) throw std::invalid_argument(w + ": bpreg must not be negative");
  s.B = (int)B, s.N = (int)N, s.S = (int)(B + N);
  return s;
}

void no_overlap(const std::string &w, const imp_matrix *const *all, int n) {
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < i; ++j)
      if (all[i]->overlaps(all[j])) throw std::invalid_argument(w + ": two of the matrices share storage");
}

// the ids of one step, checked; returns the number of active slots
int check_step(const std::string &w, const Shape &s, const int32_t *inputs, const int32_t *targets, const int32_t *negatives) {
  int active = 0;
  for (int r = 0; r < s.B; ++r) {
    if (inputs[r] < -1 || inputs[r] >= s.items) throw out_of_range_error(w + ": an input outside [-1, items)");
    if (targets[r] < -1 || targets[r] >= s.items) throw out_of_range_error(w + ": a target outside [-1, items)");
    if (inputs[r] >= 0 && targets[r] < 0) throw std::invalid_argument(w + ": an active slot with a negative target");
    active += inputs[r] >= 0;
  }
  for (int n = 0; n < s.N; ++n)
    if (negatives[n] < 0 || negatives[n] >= s.items) throw out_of_range_error(w + ": a negative outside [0, items)");
  return active;
}

// The int words of one step on the device, in this order (each run rounded up to 64 words).
struct StepWords {
  size_t inputs, reset, rows, cols, x_ids, x_start, x_occ, o_ids, o_start, o_occ, end;
  int x_n, o_n, active;
};
StepWords pack_step(const Shape &s, const int32_t *inputs, const int32_t *targets, const int32_t *reset, const int32_t *negatives,
                    int active, bool plan, std::vector<int32_t> &words) {
  StepWords at{};
  at.active = active;
  auto put = [&](const int32_t *p, size_t n) {
    const size_t first = words.size();
    words.insert(words.end(), p, p + n);
    words.resize(round64(words.size()), 0);
    return first;
  };
  std::vector<int32_t> rows(s.B), cols(s.S), fresh(s.B);
  for (int r = 0; r < s.B; ++r) rows[r] = cols[r] = inputs[r] >= 0 ? targets[r] : -1, fresh[r] = reset[r] != 0;
  std::copy(negatives, negatives + s.N, cols.begin() + s.B);
  at.inputs = put(inputs, s.B), at.reset = put(fresh.data(), s.B), at.rows = put(rows.data(), s.B), at.cols = put(cols.data(), s.S);
  if (plan) {
    const FoldPlan x = fold_plan(inputs, s.B), o = fold_plan(cols.data(), s.S);
    at.x_n = (int)x.unique.size(), at.o_n = (int)o.unique.size();
    at.x_ids = put(x.unique.data(), x.unique.size()), at.x_start = put(x.start.data(), x.start.size()), at.x_occ = put(x.occ.data(), x.occ.size());
    at.o_ids = put(o.unique.data(), o.unique.size()), at.o_start = put(o.start.data(), o.start.size()), at.o_occ = put(o.occ.data(), o.occ.size());
  }
  at.end = words.size();
  return at;
}

// the float temporaries of a step, carved from ctx().gru_ws behind the int words
struct Temps {
  float *r, *z, *c, *h0, *rh, *stats, *diag, *rowstat, *G;
  static size_t words(const Shape &s) {
    const size_t bh = (size_t)s.B * s.H;
    return 5 * bh + round64((size_t)kPlanes * (s.S / kTile) * s.B) + round64(s.B) + (size_t)s.B * 8 + (size_t)s.B * s.S;
  }
  Temps(float *p, const Shape &s) {
    const size_t bh = (size_t)s.B * s.H;
    r = p, z = r + bh, c = z + bh, h0 = c + bh, rh = h0 + bh, stats = rh + bh;
    diag = stats + round64((size_t)kPlanes * (s.S / kTile) * s.B), rowstat = diag + round64(s.B), G = rowstat + (size_t)s.B * 8;
  }
};
struct GruParams {
  const float *W_x, *W_h, *b, *W_out;
};
struct GruGradients {
  float *h1, *da, *dcol, *dh1, *dW_h, *db;
};

// queues the eight launches of one step's forward and backward pass; h1 may be h itself (imp_gru_steps)
void queue_gradients(const Shape &s, const GruParams &p, const float *h, const int32_t *words_d, const StepWords &at, float bpreg,
                     const Temps &t, const GruGradients &g, float *loss) {
  const int B = s.B, S = s.S, H = s.H, hb = (H + kTile - 1) / kTile;
  const float inv_active = at.active ? 1.0f / (float)at.active : 0.f;
  const Gates gates{h, words_d + at.inputs, words_d + at.reset, 0, B, H, p.W_x, p.W_h, p.b, t.r, t.z, t.h0, t.rh, t.c, g.h1};
  const Scores sc{g.h1, p.W_out, words_d + at.cols, words_d + at.rows, B, S, H, inv_active, bpreg, t.stats, t.diag, t.rowstat, t.G, loss};
  const Back bk{B, S, H, t.G, words_d + at.cols, p.W_out, p.W_h, g.h1, t.r, t.z, t.c, t.h0, t.rh, g.dh1, g.da, g.dcol, g.dW_h, g.db};
  const unsigned tiles = (unsigned)((B / kTile) * (S / kTile));
  {
    IMP_PROF("gru_gates");
    gru_gates_rz_kernel<<<(B / kTile) * (H / 32), 256, 0, stream()>>>(gates);
    gru_gates_c_kernel<<<(B / kTile) * hb, 256, 0, stream()>>>(gates);
  }
  {
    IMP_PROF("gru_scores");
    if (s.bpr) {
      gru_scores_kernel<1, true><<<tiles, 256, 0, stream()>>>(sc);
      gru_merge_kernel<true><<<1, 256, 0, stream()>>>(sc);
      gru_scores_kernel<2, true><<<tiles, 256, 0, stream()>>>(sc);
    } else {
      gru_scores_kernel<1, false><<<tiles, 256, 0, stream()>>>(sc);
      gru_merge_kernel<false><<<1, 256, 0, stream()>>>(sc);
      gru_scores_kernel<2, false><<<tiles, 256, 0, stream()>>>(sc);
    }
  }
  {
    IMP_PROF("gru_backward");
    gru_back_out_kernel<<<(B / kTile + S / kTile) * hb + (S + 255) / 256, 256, 0, stream()>>>(bk);
    gru_back_r_kernel<<<(B / kTile) * hb, 256, 0, stream()>>>(bk);
    gru_back_w_kernel<<<hb * ((3 * H + kTile - 1) / kTile) + (3 * H + 255) / 256, 256, 0, stream()>>>(bk);
  }
  IMP_CHECK_HIP(hipGetLastError());
}

bool shaped(const imp_matrix *m, size_t rows, size_t cols) { return m && m->itemsize == 4 && m->rows == rows && m->cols == cols; }

}  // namespace
}  // namespace imp

using namespace imp;

extern "C" int imp_host_gru_fold_plan(const int32_t *ids, int64_t n, int32_t *unique, int32_t *start, int32_t *occ, int64_t *n_unique,
                                      int64_t *n_occ) {
  return guarded_host([&] {
    if (n < 0 || n > INT32_MAX || (n && !ids) || !unique || !start || !occ || !n_unique || !n_occ) throw std::invalid_argument("gru_fold_plan: bad argument");
    const FoldPlan p = fold_plan(ids, n);
    std::copy(p.unique.begin(), p.unique.end(), unique);
    std::copy(p.start.begin(), p.start.end(), start);
    std::copy(p.occ.begin(), p.occ.end(), occ);
    *n_unique = (int64_t)p.unique.size(), *n_occ = (int64_t)p.occ.size();
  });
}

extern "C" int imp_gru_gradients(const imp_matrix *W_x, const imp_matrix *W_h, const imp_matrix *b, const imp_matrix *W_out,
                                 const imp_matrix *h, const int32_t *inputs, const int32_t *targets, const int32_t *reset,
                                 int64_t batch_size, const int32_t *negatives, int64_t n_negatives, const char *loss, float bpreg,
                                 imp_matrix *h1, imp_matrix *da, imp_matrix *dcol, imp_matrix *dh1, imp_matrix *dW_h, imp_matrix *db,
                                 float *loss_out) {
  return guarded([&] {
    const std::string w("gru_gradients");
    if (!W_x || !W_h || !b || !W_out || !h || !inputs || !targets || !reset || (n_negatives > 0 && !negatives) || !loss_out)
      throw std::invalid_argument(w + ": NULL argument");
    const Shape s = shape_of(w, W_x, W_h, b, W_out, h, batch_size, n_negatives, loss, bpreg);
    const size_t B = s.B, H = s.H;
    if (!shaped(h1, B, H) || !shaped(dh1, B, H) || !shaped(da, B, 3 * H) || !shaped(dcol, s.S, H + 1) || !shaped(dW_h, H, 3 * H) || !shaped(db, 1, 3 * H))
      throw std::invalid_argument(w + ": h1, dh1 [batch_size x hidden], da [batch_size x 3 hidden], dcol [(batch_size + negatives) x (hidden + 1)], dW_h, db must be float32 of these shapes");
    const imp_matrix *all[] = {W_x, W_h, b, W_out, h, h1, da, dcol, dh1, dW_h, db};
    no_overlap(w, all, 11);
    const int active = check_step(w, s, inputs, targets, negatives);
    std::vector<int32_t> words;
    const StepWords at = pack_step(s, inputs, targets, reset, negatives, active, false, words);
    float *ws = ctx().gru_ws.reserve(at.end + 64 + Temps::words(s));
    IMP_CHECK_HIP(hipMemcpyAsync(ws, words.data(), at.end * 4, hipMemcpyHostToDevice, stream()));
    float *loss_d = ws + at.end;
    const Temps t(loss_d + 64, s);
    queue_gradients(s, GruParams{W_x->f32(), W_h->f32(), b->f32(), W_out->f32()}, h->f32(), reinterpret_cast<const int32_t *>(ws), at, bpreg, t,
                    GruGradients{h1->mut<float>(), da->mut<float>(), dcol->mut<float>(), dh1->mut<float>(), dW_h->mut<float>(), db->mut<float>()}, loss_d);
    IMP_CHECK_HIP(hipMemcpyAsync(loss_out, loss_d, 4, hipMemcpyDeviceToHost, stream()));
    sync();
  });
}

extern "C" int imp_gru_steps(imp_matrix *const *params, imp_matrix *const *accumulators, imp_matrix *h, const int32_t *inputs,
                             const int32_t *targets, const int32_t *reset, int64_t steps, int64_t batch_size, const int32_t *negatives,
                             int64_t n_negatives, const char *loss, float bpreg, float learning_rate, float *losses) {
  return guarded([&] {
    const std::string w("gru_steps");
    if (!params || !accumulators || !h || !inputs || !targets || !reset || (n_negatives > 0 && !negatives) || !losses)
      throw std::invalid_argument(w + ": NULL argument");
    const imp_matrix *all[9];
    for (int i = 0; i < 4; ++i) all[i] = params[i], all[4 + i] = accumulators[i];
    all[8] = h;
    for (const imp_matrix *m : all)
      if (!m) throw std::invalid_argument(w + ": NULL argument");
    const Shape s = shape_of(w, params[0], params[1], params[2], params[3], h, batch_size, n_negatives, loss, bpreg);
    if (steps < 1 || steps > 65536) throw std::invalid_argument(w + ": the number of steps must lie in 1 .. 65536");
    for (int i = 0; i < 4; ++i)
      if (!shaped(accumulators[i], params[i]->rows, params[i]->cols)) throw std::invalid_argument(w + ": an accumulator must be float32 and shaped like its parameter");
    no_overlap(w, all, 9);
    const size_t B = s.B, H = s.H, N = s.N;
    std::vector<int> active(steps);
    for (int64_t t = 0; t < steps; ++t) active[t] = check_step(w, s, inputs + t * B, targets + t * B, negatives + t * N);
    std::vector<int32_t> words;
    std::vector<StepWords> at;
    for (int64_t t = 0; t < steps; ++t) at.push_back(pack_step(s, inputs + t * B, targets + t * B, reset + t * B, negatives + t * N, active[t], true, words));
    const size_t n_loss = round64(steps), grads = B * 3 * H + (size_t)s.S * (H + 1) + B * H + round64(H * 3 * H) + round64(3 * H);
    float *ws = ctx().gru_ws.reserve(words.size() + n_loss + grads + Temps::words(s));
    const int32_t *words_d = reinterpret_cast<const int32_t *>(ws);
    IMP_CHECK_HIP(hipMemcpyAsync(ws, words.data(), words.size() * 4, hipMemcpyHostToDevice, stream()));
    float *loss_d = ws + words.size(), *q = loss_d + n_loss;
    GruGradients g{};
    g.da = q, q += B * 3 * H;
    g.dcol = q, q += (size_t)s.S * (H + 1);
    g.dh1 = q, q += B * H;
    g.dW_h = q, q += round64(H * 3 * H);
    g.db = q, q += round64(3 * H);
    const Temps tmp(q, s);
    float *P[4], *A[4];
    for (int i = 0; i < 4; ++i) P[i] = params[i]->mut<float>(), A[i] = accumulators[i]->mut<float>();
    g.h1 = h->mut<float>();
    {
      IMP_PROF("gru_zero");
      gru_zero_kernel<<<1, 256, 0, stream()>>>(loss_d, n_loss);
    }
    for (int64_t t = 0; t < steps; ++t) {
      if (!at[t].active) continue;  // loss 0, nothing moves
      queue_gradients(s, GruParams{P[0], P[1], P[2], P[3]}, g.h1, words_d, at[t], bpreg, tmp, g, loss_d + t);
      IMP_PROF("gru_update");
      Update u{};
      u.x = {P[0], A[0], g.da, words_d + at[t].x_ids, words_d + at[t].x_start, words_d + at[t].x_occ, at[t].x_n, 3 * s.H};
      u.o = {P[3], A[3], g.dcol, words_d + at[t].o_ids, words_d + at[t].o_start, words_d + at[t].o_occ, at[t].o_n, s.H + 1};
      u.W_h = P[1], u.acc_W_h = A[1], u.b = P[2], u.acc_b = A[2], u.dW_h = g.dW_h, u.db = g.db;
      u.n_wh = s.H * 3 * s.H, u.n_b = 3 * s.H, u.lr = learning_rate;
      gru_update_kernel<<<(at[t].x_n + at[t].o_n + 3) / 4 + (u.n_wh + u.n_b + 255) / 256, 256, 0, stream()>>>(u);
      IMP_CHECK_HIP(hipGetLastError());
    }
    IMP_CHECK_HIP(hipMemcpyAsync(losses, loss_d, (size_t)steps * 4, hipMemcpyDeviceToHost, stream()));
    sync();
  });
}

extern "C" int imp_gru_encode(const imp_matrix *W_x, const imp_matrix *W_h, const imp_matrix *b, const int64_t *offsets,
                              const int32_t *items, int64_t n_sessions, imp_matrix *out) {
  return guarded([&] {
    const std::string w("gru_encode");
    if (!W_x || !W_h || !b || !offsets || !out) throw std::invalid_argument(w + ": NULL argument");
    const int H = hidden_of(w, W_x, W_h, b, nullptr);
    if (n_sessions < 0 || n_sessions > INT32_MAX) throw std::invalid_argument(w + ": bad session count");
    if (!shaped(out, (size_t)n_sessions, (size_t)H + 1)) throw std::invalid_argument(w + ": out must be float32, sessions x (hidden + 1)");
    for (const imp_matrix *m : {W_x, W_h, b})
      if (out->overlaps(m)) throw std::invalid_argument(w + ": out shares storage with a parameter");
    if (offsets[0] != 0) throw std::invalid_argument(w + ": offsets must start at 0");
    for (int64_t i = 0; i < n_sessions; ++i)
      if (offsets[i + 1] < offsets[i]) throw std::invalid_argument(w + ": offsets must not decrease");
    if (offsets[n_sessions] && !items) throw std::invalid_argument(w + ": NULL argument");
    for (int64_t e = 0; e < offsets[n_sessions]; ++e)
      if (items[e] < 0 || items[e] >= (int32_t)W_x->rows) throw out_of_range_error(w + ": a session item outside [0, items)");
    if (n_sessions == 0) return;
    // longest sessions first: at step t the sessions still running are a prefix
    std::vector<int32_t> order(n_sessions);
    std::iota(order.begin(), order.end(), 0);
    auto length = [&](int32_t i) { return offsets[i + 1] - offsets[i]; };
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return length(x) > length(y); });
    float *out_d = out->mut<float>();
    constexpr int64_t kChunk = 8192;  // sessions that advance together
    for (int64_t first = 0; first < n_sessions; first += kChunk) {
      const int n = (int)std::min(kChunk, n_sessions - first);
      const int64_t longest = length(order[first]);
      std::vector<int32_t> words(order.begin() + first, order.begin() + first + n);
      words.resize(round64(words.size()), 0);
      std::vector<std::pair<size_t, int>> step;  // where the step's inputs lie, how many sessions still run
      for (int64_t t = 0; t < longest; ++t) {
        int running = 0;
        while (running < n && length(order[first + running]) > t) ++running;
        step.push_back({words.size(), running});
        for (int i = 0; i < running; ++i) words.push_back(items[offsets[order[first + i]] + t]);
        words.resize(round64(words.size()), 0);
      }
      const size_t nh = round64((size_t)n * H);
      float *ws = ctx().gru_ws.reserve(words.size() + 4 * nh);
      const int32_t *words_d = reinterpret_cast<const int32_t *>(ws);
      IMP_CHECK_HIP(hipMemcpyAsync(ws, words.data(), words.size() * 4, hipMemcpyHostToDevice, stream()));
      float *hs = ws + words.size(), *z = hs + nh, *h0 = z + nh, *rh = h0 + nh;
      IMP_PROF("gru_encode");
      gru_zero_kernel<<<(unsigned)std::min<size_t>((nh + 255) / 256, 2048), 256, 0, stream()>>>(hs, nh);
      for (size_t t = 0; t < step.size(); ++t) {
        const int rows = step[t].second, row_blocks = (rows + kTile - 1) / kTile;
        const Gates gates{hs, words_d + step[t].first, nullptr, t == 0, rows, H, W_x->f32(), W_h->f32(), b->f32(), nullptr, z, h0, rh, nullptr, hs};
        gru_gates_rz_kernel<<<row_blocks * (H / 32), 256, 0, stream()>>>(gates);
        gru_gates_c_kernel<<<row_blocks * ((H + kTile - 1) / kTile), 256, 0, stream()>>>(gates);
      }
      gru_emit_kernel<<<(unsigned)(((size_t)n * (H + 1) + 255) / 256), 256, 0, stream()>>>(hs, words_d, n, H, out_d);
      IMP_CHECK_HIP(hipGetLastError());
      sync();  // the next chunk reuses the workspace, and `words` is this scope's memory
    }
  });
}
