// The kernels and host helpers of the multinomial autoencoders, shared by mult_dae.hip (which states their contract) and
// mult_vae.hip: encoder, the two decoder passes, merge, fold, bias / loss sums, scatter, dense Adam, the argument checks.
#ifndef IMPLICIT_AMD_CSRC_MULT_DAE_KERNELS_H_
#define IMPLICIT_AMD_CSRC_MULT_DAE_KERNELS_H_
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "common.h"
#include "philox.h"

namespace imp {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTile = 64;         // items per tile, batch rows per row block
constexpr int kLdg = kTile + 1;   // leading dimension of G
constexpr int kStage = 256;       // CSR entries staged per round by encode and scatter
constexpr uint32_t kTagDae = 7u;  // philox.h

__device__ __forceinline__ void store_through(float *p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void add_through(float *p, float v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// row of element e of a lane's 32 x 32 accumulator; its column is lane & 31
__device__ __forceinline__ int tile_row(int e, int lane) { return (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5); }

size_t decode_lds_bytes(int H) { return ((size_t)kTile * (H + 1) + kTile * kLdg + 4 * kTile) * 4; }

struct Batch {
  const int32_t *__restrict__ indptr;
  const int32_t *__restrict__ indices;
  const int32_t *__restrict__ rows;  // [B] row ids, -1: an empty row
  int B, H, items;
  float dropout;
  uint64_t seed;
};

// weight of the entry at CSR position pos: s when kept, 0 when dropped
__device__ __forceinline__ float entry_weight(const Batch &b, int pos, float s) {
  if (b.dropout <= 0.f) return s;
  const u32x4 r = philox4x32_10((uint32_t)pos, 0u, 0u, kTagDae, (uint32_t)b.seed, (uint32_t)(b.seed >> 32));
  return (float)(r.x >> 8) * 0x1p-24f >= b.dropout ? s : 0.f;
}

// stages the entries [lo + c, lo + c + 256) of a row: ids and weights, and whether the run is strictly ascending
__device__ __forceinline__ bool stage_entries(const Batch &b, int lo, int hi, int c, float s, int *ids, float *wts) {
  const int p = lo + c + (int)threadIdx.x;
  bool ascending = true;
  if (p < hi) {
    const int id = b.indices[p];
    ids[threadIdx.x] = id;
    wts[threadIdx.x] = entry_weight(b, p, s);
    ascending = p == lo || b.indices[p - 1] < id;
  }
  return ascending;
}

// out: h rows with leading dimension ld (ld = H + 1: column H is set to 1.0, the serving layout); hT: H x B or NULL
__global__ __launch_bounds__(256) void dae_encode_kernel(Batch b, const float *__restrict__ W_in, const float *__restrict__ b_in,
                                                         float *out, int ld, float *hT, int *unsorted) {
  __shared__ int ids[kStage];
  __shared__ float wts[kStage];
  const int r = blockIdx.x, tid = threadIdx.x, H = b.H;
  const int u = b.rows[r];
  const int lo = u < 0 ? 0 : b.indptr[u], hi = u < 0 ? 0 : b.indptr[u + 1];
  const float s = hi > lo ? 1.0f / ((1.0f - b.dropout) * sqrtf((float)(hi - lo))) : 0.f;
  const int k0 = tid, k1 = tid + 256;
  float z0 = k0 < H ? b_in[k0] : 0.f, z1 = k1 < H ? b_in[k1] : 0.f;
  bool ascending = true;
  for (int c = 0; c < hi - lo; c += kStage) {
    ascending &= stage_entries(b, lo, hi, c, s, ids, wts);
    __syncthreads();
    const int n = min(kStage, hi - lo - c);
    for (int e = 0; e < n; ++e) {
      const float w = wts[e];
      if (w == 0.f) continue;
      const float *row = W_in + (size_t)ids[e] * H;
      if (k0 < H) z0 += w * row[k0];
      if (k1 < H) z1 += w * row[k1];
    }
    __syncthreads();
  }
  if (!ascending) atomicOr(unsorted, 1);
  if (k0 < H) {
    const float h = tanhf(z0);
    store_through(out + (size_t)r * ld + k0, h);
    if (hT) store_through(hT + (size_t)k0 * b.B + r, h);
  }
  if (k1 < H) {
    const float h = tanhf(z1);
    store_through(out + (size_t)r * ld + k1, h);
    if (hT) store_through(hT + (size_t)k1 * b.B + r, h);
  }
  if (ld > H && tid == 0) store_through(out + (size_t)r * ld + H, 1.0f);
}

struct Decode {
  Batch b;
  const float *__restrict__ W_out;  // items x (H + 1)
  const float *__restrict__ h;      // B x H
  const float *__restrict__ hT;     // H x B
  float *stats;                     // three planes [tiles x B]: max, sum exp, liked logits
  const float *__restrict__ lse;    // [B], pass 2
  float *dW_out;                    // items x (H + 1), pass 2
  float *partial;                   // [grid][B x H], pass 2
  int tiles;
};

// One wavefront's 32 x 32 block of the logits of row block r0 against the W tile in the LDS: rows r0 + 32 (wave & 1) ..,
// items 32 (wave >> 1) ...  Both passes call this and nothing else, so that they form the same bits.
__device__ __forceinline__ f32x16 logit_tile(const Decode &d, const float *W, int ldw, int r0, int wave, int lane) {
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  const int l31 = lane & 31, lk = lane >> 5;
  const float *a = d.hT + (size_t)lk * d.b.B + r0 + 32 * (wave & 1) + l31;
  const float *w = W + (32 * (wave >> 1) + l31) * ldw + lk;
  const size_t step = 2 * (size_t)d.b.B;
#pragma unroll 8
  for (int ks = 0; ks < d.b.H / 2; ++ks) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ks * step], w[2 * ks], acc, 0, 0, 0);
  return acc;
}

// first position in [lo, hi) whose index is >= j
__device__ __forceinline__ int lower_bound(const int32_t *__restrict__ indices, int lo, int hi, int j) {
  int n = hi - lo;
  while (n > 0) {
    const int half = n >> 1;
    if (indices[lo + half] < j) lo += half + 1, n -= half + 1;
    else n = half;
  }
  return lo;
}

template <int PASS, int TPW> __global__ __launch_bounds__(256) void dae_decode_kernel(Decode d) {
  extern __shared__ float lds[];
  const int H = d.b.H, B = d.b.B, items = d.b.items, ldw = H + 1;
  float *W = lds, *G = W + kTile * ldw, *bias = G + kTile * kLdg;
  int *slo = reinterpret_cast<int *>(bias + kTile), *shi = slo + kTile;  // the row's first entry at or after the tile, its end
  float *srow = reinterpret_cast<float *>(shi + kTile);                    // n_u
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, lk = lane >> 5;
  const int row = tid >> 2, q = tid & 3;  // the row-wise work: four threads per row
  const float inv_b = 1.0f / (float)B;
  bool first = true;  // pass 2: the workgroup's partial dh has not been written yet

  for (int t = blockIdx.x; t < d.tiles; t += gridDim.x) {
    const int j0 = t * kTile;
    for (int j = tid >> 5; j < kTile; j += 8)
      for (int k = l31; k < H; k += 32) W[j * ldw + k] = j0 + j < items ? d.W_out[(size_t)(j0 + j) * ldw + k] : 0.f;
    if (tid < kTile) bias[tid] = j0 + tid < items ? d.W_out[(size_t)(j0 + tid) * ldw + H] : -INFINITY;
    f32x16 acc[TPW];  // pass 2: g^T h for the blocks (item half wave & 1, columns 32 ((wave >> 1) + 2 i))
#pragma unroll
    for (int i = 0; i < TPW; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
    float gb = 0.f;  // pass 2, threads 0 .. 63: the bias gradient of item j0 + tid
    __syncthreads();

    for (int r0 = 0; r0 < B; r0 += kTile) {
      {
        const f32x16 z = logit_tile(d, W, ldw, r0, wave, lane);
        const int c = 32 * (wave >> 1) + l31;
        const float bj = bias[c];  // -inf beyond the last item: such a column takes no part in any row's softmax
#pragma unroll
        for (int e = 0; e < 16; ++e) G[(32 * (wave & 1) + tile_row(e, lane)) * kLdg + c] = z[e] + bj;
      }
      if (q == 0) {
        const int u = d.b.rows[r0 + row];
        const int lo = u < 0 ? 0 : d.b.indptr[u], hi = u < 0 ? 0 : d.b.indptr[u + 1];
        slo[row] = lower_bound(d.b.indices, lo, hi, j0), shi[row] = hi;
        srow[row] = (float)(hi - lo);
      }
      __syncthreads();
      float *Gr = G + row * kLdg;
      const int first_liked = slo[row], hi = shi[row];
      if (PASS == 1) {
        float m = -INFINITY;
#pragma unroll
        for (int k = 0; k < 16; ++k) m = fmaxf(m, Gr[q + 4 * k]);
        m = fmaxf(m, __shfl_xor(m, 1));
        m = fmaxf(m, __shfl_xor(m, 2));  // finite: every tile holds at least one item
        float sum = 0.f, liked = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) sum += expf(Gr[q + 4 * k] - m);
        for (int p = first_liked + q; p < hi; p += 4) {
          const int j = d.b.indices[p] - j0;
          if (j >= kTile) break;
          if (j >= 0) liked += Gr[j];
        }
        sum += __shfl_xor(sum, 1), liked += __shfl_xor(liked, 1);
        sum += __shfl_xor(sum, 2), liked += __shfl_xor(liked, 2);
        if (q == 0) {
          const size_t at = (size_t)t * B + r0 + row, plane = (size_t)d.tiles * B;
          store_through(d.stats + at, m);
          store_through(d.stats + plane + at, sum);
          store_through(d.stats + 2 * plane + at, liked);
        }
      } else {
        const float n_u = srow[row], l = d.lse[r0 + row];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const int c = q + 4 * k;
          Gr[c] = j0 + c < items ? n_u * expf(Gr[c] - l) * inv_b : 0.f;
        }
        __syncthreads();  // the row's liked entries lie in its other threads' columns
        for (int p = first_liked + q; p < hi; p += 4) {
          const int j = d.b.indices[p] - j0;
          if (j >= kTile) break;
          if (j >= 0) Gr[j] -= inv_b;
        }
        __syncthreads();
        if (tid < kTile) {
#pragma unroll 8
          for (int r = 0; r < kTile; ++r) gb += G[r * kLdg + tid];
        }
        // g^T h: A[m = item][k = row] from G, B[k = row][n = column] from h in memory
        {
          const float *Ga = G + lk * kLdg + 32 * (wave & 1) + l31;
          const float *hb = d.h + (size_t)(r0 + lk) * H + 32 * (wave >> 1) + l31;
#pragma unroll 4
          for (int ks = 0; ks < kTile / 2; ++ks) {
            const float av = Ga[2 * ks * kLdg];
#pragma unroll
            for (int i = 0; i < TPW; ++i)
              if (32 * ((wave >> 1) + 2 * i) < H)
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, hb[(size_t)2 * ks * H + 64 * i], acc[i], 0, 0, 0);
          }
        }
        // g W: A[m = row][k = item] from G, B[k = item][n = column] from the W tile; rows 32 (wave & 1) .. of the block
        float *mine = d.partial + (size_t)blockIdx.x * B * H;
        for (int nb = wave >> 1; 32 * nb < H; nb += 2) {
          f32x16 dh;
#pragma unroll
          for (int e = 0; e < 16; ++e) dh[e] = 0.f;
          const float *Ga = G + (32 * (wave & 1) + l31) * kLdg + lk, *Wb = W + lk * ldw + 32 * nb + l31;
#pragma unroll 8
          for (int ks = 0; ks < kTile / 2; ++ks) dh = __builtin_amdgcn_mfma_f32_32x32x2f32(Ga[2 * ks], Wb[2 * ks * ldw], dh, 0, 0, 0);
          float *dst = mine + (size_t)(r0 + 32 * (wave & 1)) * H + 32 * nb + l31;
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            float *p = dst + (size_t)tile_row(e, lane) * H;
            *p = first ? dh[e] : *p + dh[e];
          }
        }
      }
      __syncthreads();  // G and the row words have been consumed
    }

    if (PASS == 2) {
      first = false;
#pragma unroll
      for (int i = 0; i < TPW; ++i) {
        const int c = 32 * ((wave >> 1) + 2 * i) + l31;
        if (c < H)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int j = j0 + 32 * (wave & 1) + tile_row(e, lane);
            if (j < items) store_through(d.dW_out + (size_t)j * ldw + c, acc[i][e]);
          }
      }
      if (tid < kTile && j0 + tid < items) store_through(d.dW_out + (size_t)(j0 + tid) * ldw + H, gb);
    }
    __syncthreads();  // the W tile has been consumed
  }
}

// one wavefront per batch row: lse and the row's loss term from the tiles' triples
__global__ __launch_bounds__(256) void dae_merge_kernel(Batch b, const float *__restrict__ stats, int tiles, float *lse, float *row_loss) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= b.B) return;
  const size_t plane = (size_t)tiles * b.B;
  float m = -INFINITY, s = 0.f, liked = 0.f;
  for (int t = lane; t < tiles; t += 64) {
    const float mt = stats[(size_t)t * b.B + r], st = stats[plane + (size_t)t * b.B + r];
    const float top = fmaxf(m, mt);
    s = s * expf(m - top) + st * expf(mt - top);  // m = -inf, s = 0 at the start: 0 * 0
    m = top;
    liked += stats[2 * plane + (size_t)t * b.B + r];
  }
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) {
    const float mo = __shfl_xor(m, x), so = __shfl_xor(s, x);
    const float top = fmaxf(m, mo);
    // a lane without a tile holds (-inf, 0); two of them stay (-inf, 0) without forming -inf - -inf
    s = top == -INFINITY ? 0.f : s * expf(m - top) + so * expf(mo - top);
    m = top;
    liked += __shfl_xor(liked, x);
  }
  if (lane == 0) {
    const int u = b.rows[r];
    const float n_u = u < 0 ? 0.f : (float)(b.indptr[u + 1] - b.indptr[u]);
    const float l = m + logf(s);
    lse[r] = l;
    row_loss[r] = n_u > 0.f ? n_u * l - liked : 0.f;
  }
}

// dh = the partials in ascending workgroup order; dz = dh (1 - h^2)
__global__ __launch_bounds__(256) void dae_fold_kernel(const float *__restrict__ partial, int parts, size_t n, const float *__restrict__ h,
                                                       float *dh, float *dz) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float s = partial[i];
  for (int g = 1; g < parts; ++g) s += partial[(size_t)g * n + i];
  const float hv = h[i];
  dh[i] = s;
  dz[i] = s * (1.0f - hv * hv);
}

// threads 0 .. H - 1 of the blocks: db_in[k] = sum_r dz[r][k] in ascending r; the last block's first wavefront: the loss
__global__ __launch_bounds__(256) void dae_bias_loss_kernel(const float *__restrict__ dz, int B, int H, float *db_in,
                                                            const float *__restrict__ row_loss, float *loss) {
  if (blockIdx.x == gridDim.x - 1) {
    const int lane = threadIdx.x;
    if (lane >= 64) return;
    float s = 0.f;
    for (int r = lane; r < B; r += 64) s += row_loss[r];
#pragma unroll
    for (int x = 1; x < 64; x <<= 1) s += __shfl_xor(s, x);
    if (lane == 0) *loss = s / (float)B;
    return;
  }
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= H) return;
  float s = 0.f;
  for (int r = 0; r < B; ++r) s += dz[(size_t)r * H + k];
  store_through(db_in + k, s);
}

__global__ __launch_bounds__(256) void dae_zero_kernel(float *p, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) store_through(p + i, 0.f);
}

// dW_in[i] += s_u m_ui dz_u for the entries of batch row blockIdx.x
__global__ __launch_bounds__(256) void dae_scatter_kernel(Batch b, const float *__restrict__ dz, float *dW_in) {
  __shared__ int ids[kStage];
  __shared__ float wts[kStage];
  const int r = blockIdx.x, tid = threadIdx.x, H = b.H;
  const int u = b.rows[r];
  if (u < 0) return;
  const int lo = b.indptr[u], hi = b.indptr[u + 1];
  if (hi == lo) return;
  const float s = 1.0f / ((1.0f - b.dropout) * sqrtf((float)(hi - lo)));
  const int k0 = tid, k1 = tid + 256;
  const float d0 = k0 < H ? dz[(size_t)r * H + k0] : 0.f, d1 = k1 < H ? dz[(size_t)r * H + k1] : 0.f;
  for (int c = 0; c < hi - lo; c += kStage) {
    stage_entries(b, lo, hi, c, s, ids, wts);
    __syncthreads();
    const int n = min(kStage, hi - lo - c);
    for (int e = 0; e < n; ++e) {
      const float w = wts[e];
      if (w == 0.f) continue;
      float *row = dW_in + (size_t)ids[e] * H;
      if (k0 < H) add_through(row + k0, w * d0);
      if (k1 < H) add_through(row + k1, w * d1);
    }
    __syncthreads();
  }
}

struct AdamSegment {
  float *p, *m, *v;
  const float *g;
  size_t n;
  int ld, decay_cols;  // reg applies to the columns below decay_cols of rows ld wide
};
struct AdamArgs {
  AdamSegment seg[3];
  float lr, b1, b2, eps, reg, c1, c2;
  const int *unsorted;
};

__global__ __launch_bounds__(256) void dae_adam_kernel(AdamArgs a) {
  if (*a.unsorted) return;
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const AdamSegment &x = a.seg[s];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < x.n; i += (size_t)gridDim.x * 256) {
      const float p = x.p[i];
      float g = x.g[i];
      if ((int)(i % (size_t)x.ld) < x.decay_cols) g += a.reg * p;
      const float m = a.b1 * x.m[i] + (1.0f - a.b1) * g;
      const float v = a.b2 * x.v[i] + (1.0f - a.b2) * (g * g);
      store_through(x.m + i, m);
      store_through(x.v + i, v);
      store_through(x.p + i, p - a.lr * (m * a.c1) / (sqrtf(v * a.c2) + a.eps));
    }
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
size_t round64(size_t n) { return (n + 63) / 64 * 64; }

int hidden_of(const std::string &w, const imp_csr *C, const imp_matrix *W_in, const imp_matrix *b_in, const imp_matrix *W_out) {
  if (!C->parts.empty()) throw std::invalid_argument(w + ": a CSR held in several blocks (more than 2^31 - 1 nonzeros) is not supported");
  if (W_in->itemsize != 4 || b_in->itemsize != 4 || (W_out && W_out->itemsize != 4)) throw std::invalid_argument(w + ": parameters must be float32");
  const size_t H = W_in->cols;
  if (H < 32 || H > 512 || H % 32) throw std::invalid_argument(w + ": hidden must be a multiple of 32 in 32 .. 512");
  if (W_in->rows != (size_t)C->cols) throw std::invalid_argument(w + ": W_in must have one row per column of user_items");
  if (b_in->rows != 1 || b_in->cols != H) throw std::invalid_argument(w + ": b_in must be 1 x hidden");
  if (W_out && (W_out->rows != W_in->rows || W_out->cols != H + 1)) throw std::invalid_argument(w + ": W_out must be items x (hidden + 1)");
  return (int)H;
}

void check_rows(const std::string &w, const imp_csr *C, const int32_t *rows, int64_t n) {
  if (!rows && n) throw std::invalid_argument(w + ": NULL row ids");
  for (int64_t r = 0; r < n; ++r)
    if (rows[r] < -1 || rows[r] >= C->rows) throw out_of_range_error(w + ": row id outside user_items");
}

void same_shape(const std::string &w, const imp_matrix *a, const imp_matrix *like, const char *name) {
  if (!a || a->itemsize != 4 || a->rows != like->rows || a->cols != like->cols) throw std::invalid_argument(w + ": " + name + " must be float32 and shaped like its parameter");
}

struct Gradients {
  float *dW_in, *db_in, *dW_out, *dh, *dz;  // all NULL: the five arrays are taken from the workspace (imp_dae_step)
};

// What a queued batch leaves behind on the device: the loss, the encoder's unsorted flag (the word after it), the gradients.
struct Queued {
  const float *loss;
  const int *unsorted;
  Gradients g;
};
// Queues forward and backward of one batch on the library stream.
Queued queue_gradients(const imp_csr *C, const int32_t *rows, int B, int H, const float *W_in, const float *b_in, const float *W_out,
                       float dropout, uint64_t seed, Gradients g) {
  const int items = C->cols, tiles = (items + kTile - 1) / kTile;
  const int grid = std::min(tiles, std::max(1, ctx().num_cus));
  const size_t bh = (size_t)B * H, stats_n = round64(3 * (size_t)tiles * B);
  const size_t n_in = (size_t)items * H, n_out = (size_t)items * (H + 1);
  const bool own = !g.dW_in;
  const size_t need = round64(B) + 2 * bh + stats_n + 2 * round64(B) + 64 + (size_t)grid * bh +
                      (own ? 2 * bh + round64(n_in) + round64(H) + round64(n_out) : 0);
  float *ws = ctx().dae_ws.reserve(need);
  int32_t *rows_d = reinterpret_cast<int32_t *>(ws);
  float *h = ws + round64(B), *hT = h + bh, *stats = hT + bh, *lse = stats + stats_n;
  float *row_loss = lse + round64(B), *loss = row_loss + round64(B), *partial = loss + 64;
  int *unsorted = reinterpret_cast<int *>(loss + 1);
  if (own) {
    float *p = partial + (size_t)grid * bh;
    g = {p + 2 * bh, p + 2 * bh + round64(n_in), p + 2 * bh + round64(n_in) + round64(H), p, p + bh};
  }
  float *dh = g.dh, *dz = g.dz;
  IMP_CHECK_HIP(hipMemcpyAsync(rows_d, rows, (size_t)B * 4, hipMemcpyHostToDevice, stream()));
  IMP_CHECK_HIP(hipMemsetAsync(loss, 0, 64 * 4, stream()));
  const Batch b{C->indptr.data(), C->indices.data(), rows_d, B, H, items, dropout, seed};
  {
    IMP_PROF("dae_encode");
    dae_encode_kernel<<<B, 256, 0, stream()>>>(b, W_in, b_in, h, H, hT, unsorted);
    IMP_CHECK_HIP(hipGetLastError());
  }
  const Decode d{b, W_out, h, hT, stats, lse, g.dW_out, partial, tiles};
  const size_t lds = decode_lds_bytes(H);
  {
    IMP_PROF("dae_pass1");
    allow_dynamic_lds(dae_decode_kernel<1, 1>, lds);
    dae_decode_kernel<1, 1><<<grid, 256, lds, stream()>>>(d);
    dae_merge_kernel<<<(B + 3) / 4, 256, 0, stream()>>>(b, stats, tiles, lse, row_loss);
    IMP_CHECK_HIP(hipGetLastError());
  }
  {
    IMP_PROF("dae_pass2");
    auto launch = [&](auto kernel) {
      allow_dynamic_lds(kernel, lds);
      kernel<<<grid, 256, lds, stream()>>>(d);
    };
    switch ((H + 63) / 64) {  // accumulators of g^T h per wavefront: 2 H / 32 blocks over 4 wavefronts
      case 1: launch(dae_decode_kernel<2, 1>); break;
      case 2: launch(dae_decode_kernel<2, 2>); break;
      case 3:
      case 4: launch(dae_decode_kernel<2, 4>); break;
      default: launch(dae_decode_kernel<2, 8>); break;
    }
    IMP_CHECK_HIP(hipGetLastError());
  }
  {
    IMP_PROF("dae_rest");
    dae_fold_kernel<<<(unsigned)((bh + 255) / 256), 256, 0, stream()>>>(partial, grid, bh, h, dh, dz);
    dae_bias_loss_kernel<<<(H + 255) / 256 + 1, 256, 0, stream()>>>(dz, B, H, g.db_in, row_loss, loss);
    dae_zero_kernel<<<(unsigned)std::min<size_t>((n_in + 255) / 256, (size_t)ctx().num_cus * 8), 256, 0, stream()>>>(g.dW_in, n_in);
    dae_scatter_kernel<<<B, 256, 0, stream()>>>(b, dz, g.dW_in);
    IMP_CHECK_HIP(hipGetLastError());
  }
  return {loss, unsorted, g};
}

// waits for the stream; the loss, or invalid_argument when the encoder met a row that is not strictly ascending
float finish(const std::string &w, const Queued &q) {
  float host[2];
  IMP_CHECK_HIP(hipMemcpyAsync(host, q.loss, sizeof(host), hipMemcpyDeviceToHost, stream()));
  sync();
  int flag;
  memcpy(&flag, host + 1, sizeof(flag));
  if (flag) throw std::invalid_argument(w + ": a row of user_items is not strictly ascending (sort_indices / sum_duplicates first)");
  return host[0];
}

void check_batch(const std::string &w, int64_t B, float dropout) {
  if (B < 64 || B % 64 || B > (1 << 20)) throw std::invalid_argument(w + ": batch_size must be a multiple of 64");
  if (!(dropout >= 0.f && dropout < 1.f)) throw std::invalid_argument(w + ": dropout must lie in [0, 1)");
}

}  // namespace
}  // namespace imp
#endif  // IMPLICIT_AMD_CSRC_MULT_DAE_KERNELS_H_
