// K26: Mult-VAE -- the variational autoencoder of Liang, Krishnan, Hoffman and Jebara, "Variational Autoencoders for
// Collaborative Filtering" (WWW 2018, Mult-VAE^PR), one tanh layer on either side of a Gaussian code: imp_vae_encode,
// imp_vae_gradients, imp_vae_step.  Encoder, decoder passes, merge, fold, scatter and Adam are mult_dae.hip's kernels
// (mult_dae_kernels.h), unchanged; this file adds what lies between encoder and decoder.
//
// No reference counterpart.  All parameters are float32:  W_in [items x H], b_in [1 x H] (as Mult-DAE);  W_lat [H x 2L], b_lat
// [1 x 2L], columns 0 .. L - 1 for mu, L .. 2L - 1 for the log-variance lv;  W_dec [L x H], b_dec [1 x H];  W_out [items x (H + 1)],
// bias last.  H a multiple of 32 in 32 .. 512, L a multiple of 32 in 32 .. 256, a batch is B row ids, B a multiple of 64.
//   forward, batch slot r holding row u (n_u stored entries; u = -1 or n_u = 0: an empty row):
//     h1  = tanh(z1), the Mult-DAE encoder (dropout mask from Philox tag 7, s_u = 1 / ((1 - p) sqrt(n_u)));
//     a   = b_lat + h1 W_lat, one fp32 chain per element in ascending k, the bias added last;  mu = a[:L], lv = a[L:];
//     eps = 0 when sample = 0; otherwise R = Philox4x32-10(counter (r, l, 0, 8), key = seed), u1 = (float(R.x >> 8) + 0.5f) 2^-24,
//           u2 = float(R.y >> 8) 2^-24, eps = sqrtf(-2 logf(u1)) cosf(2 pi u2)  (2 pi as float32, the product in float32);
//     z   = mu + eps exp(0.5 lv)  (z = mu itself when sample = 0);   h2 = tanh(b_dec + z W_dec), the bias added last;
//     logits, lse and the multinomial NLL from h2 as Mult-DAE forms them from h;
//     KL  = (1 / B) sum over non-empty rows of sum_l 0.5 (((exp(lv) + mu^2) - 1) - lv);   loss = NLL + beta KL.
//   backward: dz2 = dh2 (1 - h2^2) from the fold;  db_dec = sum_r dz2;  dW_dec = z^T dz2;  dzl = dz2 W_dec^T;
//     dmu = dzl + (beta / B) mu;   dlv = ((0.5 dzl) eps) exp(0.5 lv) + (beta / 2B) (exp(lv) - 1);  both 0 for an empty row;
//     da = [dmu | dlv];  db_lat = sum_r da;  dW_lat = h1^T da;  dh1 = da W_lat^T;  dz1 = dh1 (1 - h1^2);  db_in = sum_r dz1;
//     dW_in by the Mult-DAE scatter of dz1.  Adam as Mult-DAE over the seven parameters, weight decay on the four weight
//     matrices (W_out's bias column excepted), none on the biases.
//
// Kernels (256 threads = 4 wavefronts).  Every product is a 64 x 64 output block per workgroup, one 32 x 32 accumulator of
// v_mfma_f32_32x32x2_f32 per wavefront (rows 32 (wave & 1), columns 32 (wave >> 1)), one chain per element in ascending k.
// Both operands move through the LDS in chunks of 32 k, loaded into registers one chunk ahead of the products (block_product).
//   latent    grid (B / 64) x (L / 32): a workgroup forms mu and lv of 64 rows x 32 code columns -- its "64 columns" are 32 of
//             mu and the same 32 of lv, so that the epilogue has both halves of an element: bias, the Philox draw, z, and the
//             row's KL terms of these 32 columns summed by an xor butterfly over 32 lanes.  Writes mu | lv, eps, z and the KL
//             partial [column block][row].  Split by column block because B / 64 alone is 8 workgroups at B = 512.
//   hidden    grid (B / 64) x (H / 64): h2 = tanh(b_dec + z W_dec), K = L; writes h2 and the transpose h2T (the decoder's A
//             operand).  Workgroup 0's first wavefront then sums the KL partials: per row the column blocks ascending, lane l
//             the rows l, l + 64, ..., the lanes by an xor butterfly.
//   backward<1>, after the fold: the row-wise product dzl = dz2 W_dec^T with the KL gradient as its epilogue (writes da), the
//             batch-reducing product dW_dec = z^T dz2 (K = B) split over its OUTPUT blocks, each one chain in ascending batch
//             order, and db_dec as column sums of dz2 in ascending row order -- three kinds of workgroup in one launch.
//   backward<2>: the same kernel on the next layer: dh1 = da W_lat^T with the factor (1 - h1^2) as epilogue (writes dz1),
//             dW_lat = h1^T da, db_lat.  Then Mult-DAE's bias / loss kernel takes db_in from dz1 and sums the NLL.
// Launches: encoder, latent, hidden, pass 1 (two between encoder and decoder); fold, backward<1>, backward<2>, bias / loss,
// scatter (three between fold and scatter: dW_in is zeroed before the encoder).  No floating-point atomics in this file's
// kernels; everything but dW_in is bit-reproducible on one device.
//
// LDS of a product: two panels of 2112 words.  A panel that lies in memory with k as its row index (W_lat and W_dec forwards,
// z and h1 and the incoming gradients in the dW products) is stored [k][64] with leading dimension 65; one that lies with k as
// its column index (h1, z, dz2, da row-wise; W_dec and W_lat backwards, read transposed) is stored [64][k] with leading
// dimension 33.  The matrix instruction reads 32 rows or columns of one k per half-wavefront: 32 consecutive words of the first
// kind, 32 words 33 apart of the second, 32 banks either way, so the same copy of a weight panel serves the forward and the
// transposed product without a conflict.  The latent kernel adds a 64 x 65 plane for mu | lv: 33 792 bytes in all.
//
// Visibility: whatever a later kernel reads is written with agent-scope stores.  Every address is bounded:
// block rows and columns beyond the matrix are loaded as 0 and never stored, K is a multiple of 32 in every product.
#include "mult_dae_kernels.h"

namespace imp {
namespace {

constexpr int kKc = 32;                 // k per staged chunk
constexpr int kLdK = kKc + 1;           // a panel stored [64][k]
constexpr int kLdT = kTile + 1;         // a panel stored [k][64]
constexpr int kPanel = kTile * kLdK;    // 2112 words >= 32 x 65
constexpr uint32_t kTagVae = 8u;        // philox.h

// One operand of a block product as it lies in memory: the 64 rows (A) or columns (B) of the block are at0 .. at0 + 31 and
// at1 .. at1 + 31 of the stored matrix, those at or beyond `extent` do not exist.
struct Panel {
  const float *__restrict__ p;
  int ld, extent, at0, at1;
};

// KMAJOR: the matrix is stored with k as its row index
template <bool KMAJOR> __device__ __forceinline__ void panel_load(const Panel &x, int k0, float (&r)[8]) {
  const int tid = threadIdx.x;
  if (KMAJOR) {
    const int i = tid & 63, at = i < 32 ? x.at0 + i : x.at1 + i - 32;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = at < x.extent ? x.p[(size_t)(k0 + (tid >> 6) + 4 * j) * x.ld + at] : 0.f;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i = (tid >> 5) + 8 * j, at = i < 32 ? x.at0 + i : x.at1 + i - 32;
      r[j] = at < x.extent ? x.p[(size_t)at * x.ld + k0 + (tid & 31)] : 0.f;
    }
  }
}
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
template <bool AK, bool BK> __device__ __forceinline__ f32x16 block_product(const Panel &A, const Panel &Bp, int K, float *As, float *Bs) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, lk = lane >> 5;
  const int mw = 32 * (wave & 1) + l31, nw = 32 * (wave >> 1) + l31;
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  float ra[8], rb[8];
  panel_load<AK>(A, 0, ra);
  panel_load<BK>(Bp, 0, rb);
  for (int k0 = 0; k0 < K; k0 += kKc) {
    panel_store<AK>(As, ra);
    panel_store<BK>(Bs, rb);
    __syncthreads();
    if (k0 + kKc < K) {
      panel_load<AK>(A, k0 + kKc, ra);
      panel_load<BK>(Bp, k0 + kKc, rb);
    }
#pragma unroll
    for (int ks = 0; ks < kKc / 2; ++ks)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(panel_read<AK>(As, mw, 2 * ks + lk), panel_read<BK>(Bs, nw, 2 * ks + lk), acc, 0, 0, 0);
    __syncthreads();
  }
  return acc;
}

struct Latent {
  Batch b;                          // b.B: the rows of this call (any number for imp_vae_encode)
  const float *__restrict__ h1;     // rows x H
  const float *__restrict__ W_lat;  // H x 2L
  const float *__restrict__ b_lat;  // 2L
  int L, sample;
  float *mu_lv, *eps, *z;           // rows x 2L, rows x L, rows x L
  float *kl_part;                   // [L / 32][rows]
};

__device__ __forceinline__ bool live_row(const Batch &b, int r) {
  const int u = b.rows[r];
  return u >= 0 && b.indptr[u + 1] > b.indptr[u];
}

__global__ __launch_bounds__(256) void vae_latent_kernel(Latent a) {
  __shared__ float As[kPanel], Bs[kPanel], Cs[kTile * kLdT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31;
  const int L = a.L, H = a.b.H, rows = a.b.B, blocks = L / 32;
  const int m0 = (int)(blockIdx.x / blocks) * kTile, cb = blockIdx.x % blocks;
  const Panel A{a.h1, H, rows, m0, m0 + 32}, W{a.W_lat, 2 * L, 2 * L, 32 * cb, L + 32 * cb};
  const f32x16 acc = block_product<false, true>(A, W, H, As, Bs);
  {
    const int n = 32 * (wave >> 1) + l31;
    const float bias = a.b_lat[(wave >> 1 ? L : 0) + 32 * cb + l31];
#pragma unroll
    for (int e = 0; e < 16; ++e) Cs[(32 * (wave & 1) + tile_row(e, lane)) * kLdT + n] = acc[e] + bias;
  }
  __syncthreads();
  const int l = 32 * cb + l31;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int row = (tid >> 5) + 8 * i, r = m0 + row;
    float term = 0.f;
    if (r < rows) {
      const float mu = Cs[row * kLdT + l31], lv = Cs[row * kLdT + 32 + l31];
      float eps = 0.f, z = mu;
      if (a.sample) {
        const u32x4 R = philox4x32_10((uint32_t)r, (uint32_t)l, 0u, kTagVae, (uint32_t)a.b.seed, (uint32_t)(a.b.seed >> 32));
        const float u1 = ((float)(R.x >> 8) + 0.5f) * 0x1p-24f, u2 = (float)(R.y >> 8) * 0x1p-24f;
        eps = sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
        z = mu + eps * expf(0.5f * lv);
      }
      store_through(a.mu_lv + (size_t)r * 2 * L + l, mu);
      store_through(a.mu_lv + (size_t)r * 2 * L + L + l, lv);
      store_through(a.eps + (size_t)r * L + l, eps);
      store_through(a.z + (size_t)r * L + l, z);
      term = live_row(a.b, r) ? 0.5f * (((expf(lv) + mu * mu) - 1.0f) - lv) : 0.f;
    }
#pragma unroll
    for (int x = 1; x < 32; x <<= 1) term += __shfl_xor(term, x);
    if (l31 == 0 && r < rows) store_through(a.kl_part + (size_t)cb * rows + r, term);
  }
}

struct Hidden {
  const float *__restrict__ z;      // rows x L
  const float *__restrict__ W_dec;  // L x H
  const float *__restrict__ b_dec;  // H
  int rows, L, H;
  float *out;                       // rows x ld; ld = H + 1: column H is set to 1.0, the serving layout
  int ld;
  float *h2T;                       // H x rows or NULL
  const float *__restrict__ kl_part;
  float *kl;                        // or NULL
};

__global__ __launch_bounds__(256) void vae_hidden_kernel(Hidden a) {
  __shared__ float As[kPanel], Bs[kPanel];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31;
  const int H = a.H, L = a.L, rows = a.rows, blocks = (H + kTile - 1) / kTile;
  const int m0 = (int)(blockIdx.x / blocks) * kTile, n0 = (int)(blockIdx.x % blocks) * kTile;
  const Panel A{a.z, L, rows, m0, m0 + 32}, W{a.W_dec, H, H, n0, n0 + 32};
  const f32x16 acc = block_product<false, true>(A, W, L, As, Bs);
  const int c = n0 + 32 * (wave >> 1) + l31;
  if (c < H) {
    const float bias = a.b_dec[c];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int r = m0 + 32 * (wave & 1) + tile_row(e, lane);
      if (r >= rows) continue;
      const float h = tanhf(acc[e] + bias);
      store_through(a.out + (size_t)r * a.ld + c, h);
      if (a.h2T) store_through(a.h2T + (size_t)c * rows + r, h);
    }
  }
  if (a.ld > H && n0 == 0 && tid < kTile && m0 + tid < rows) store_through(a.out + (size_t)(m0 + tid) * a.ld + H, 1.0f);
  if (a.kl && blockIdx.x == 0 && wave == 0) {
    float s = 0.f;
    for (int r = lane; r < rows; r += 64) {
      float t = 0.f;
      for (int cb = 0; cb < L / 32; ++cb) t += a.kl_part[(size_t)cb * rows + r];
      s += t;
    }
#pragma unroll
    for (int x = 1; x < 64; x <<= 1) s += __shfl_xor(s, x);
    if (lane == 0) *a.kl = s / (float)rows;
  }
}

// One layer of the backward pass.  G [B x gc] is the gradient that arrives (dz2, gc = H; da, gc = 2L), W [oc x gc] the layer's
// weights (W_dec, oc = L; W_lat, oc = H), X [B x oc] what the layer was fed (z; h1).
struct Backward {
  Batch b;
  const float *__restrict__ G;
  const float *__restrict__ W;
  const float *__restrict__ X;
  int gc, oc;
  float *dW, *db;                    // oc x gc, gc
  float *out;                        // stage 1: da [B x 2 oc];  stage 2: dz1 [B x oc]
  const float *__restrict__ mu_lv;   // stage 1
  const float *__restrict__ eps;     // stage 1
  float kl_scale;                    // stage 1: beta / B
};

template <int STAGE> __global__ __launch_bounds__(256) void vae_backward_kernel(Backward a) {
  __shared__ float As[kPanel], Bs[kPanel];
  __shared__ int live[kTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31;
  const int B = a.b.B, gc = a.gc, oc = a.oc;
  const int oc_blocks = (oc + kTile - 1) / kTile, gc_blocks = (gc + kTile - 1) / kTile;
  const int row_wise = (B / kTile) * oc_blocks, weights = oc_blocks * gc_blocks;
  int id = blockIdx.x;
  if (id < row_wise) {  // out = epilogue(G W^T)
    const int m0 = (id / oc_blocks) * kTile, n0 = (id % oc_blocks) * kTile;
    if (STAGE == 1 && tid < kTile) live[tid] = live_row(a.b, m0 + tid);  // the product's barriers order it before the epilogue
    const Panel A{a.G, gc, B, m0, m0 + 32}, W{a.W, gc, oc, n0, n0 + 32};
    const f32x16 acc = block_product<false, false>(A, W, gc, As, Bs);
    const int c = n0 + 32 * (wave >> 1) + l31;
    if (c >= oc) return;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = 32 * (wave & 1) + tile_row(e, lane), r = m0 + row;
      if (STAGE == 1) {
        float dmu = 0.f, dlv = 0.f;
        if (live[row]) {
          const float mu = a.mu_lv[(size_t)r * 2 * oc + c], lv = a.mu_lv[(size_t)r * 2 * oc + oc + c];
          dmu = acc[e] + a.kl_scale * mu;
          dlv = ((0.5f * acc[e]) * a.eps[(size_t)r * oc + c]) * expf(0.5f * lv) + (0.5f * a.kl_scale) * (expf(lv) - 1.0f);
        }
        store_through(a.out + (size_t)r * 2 * oc + c, dmu);
        store_through(a.out + (size_t)r * 2 * oc + oc + c, dlv);
      } else {
        const float h = a.X[(size_t)r * oc + c];
        store_through(a.out + (size_t)r * oc + c, acc[e] * (1.0f - h * h));
      }
    }
    return;
  }
  id -= row_wise;
  if (id < weights) {  // dW = X^T G: one chain per element over the batch, ascending
    const int m0 = (id / gc_blocks) * kTile, n0 = (id % gc_blocks) * kTile;
    const Panel A{a.X, oc, oc, m0, m0 + 32}, Gp{a.G, gc, gc, n0, n0 + 32};
    const f32x16 acc = block_product<true, true>(A, Gp, B, As, Bs);
    const int c = n0 + 32 * (wave >> 1) + l31;
    if (c >= gc) return;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int m = m0 + 32 * (wave & 1) + tile_row(e, lane);
      if (m < oc) store_through(a.dW + (size_t)m * gc + c, acc[e]);
    }
    return;
  }
  id -= weights;
  const int c = id * 256 + tid;  // db = the column sums of G, rows ascending
  if (c >= gc) return;
  float s = 0.f;
  for (int r = 0; r < B; ++r) s += a.G[(size_t)r * gc + c];
  store_through(a.db + c, s);
}

template <int STAGE> void launch_backward(const Backward &a) {
  const int oc_blocks = (a.oc + kTile - 1) / kTile, gc_blocks = (a.gc + kTile - 1) / kTile;
  const int grid = (a.b.B / kTile) * oc_blocks + oc_blocks * gc_blocks + (a.gc + 255) / 256;
  vae_backward_kernel<STAGE><<<grid, 256, 0, stream()>>>(a);
}

// ---- host side -------------------------------------------------------------------------------------------------------------
struct VaeParams {
  const float *W_in, *b_in, *W_lat, *b_lat, *W_dec, *b_dec, *W_out;
};

// checks the seven parameters against each other; returns L
int latent_of(const std::string &w, int H, const imp_matrix *W_lat, const imp_matrix *b_lat, const imp_matrix *W_dec, const imp_matrix *b_dec) {
  for (const imp_matrix *m : {W_lat, b_lat, W_dec, b_dec})
    if (m->itemsize != 4) throw std::invalid_argument(w + ": parameters must be float32");
  const size_t L = W_dec->rows;
  if (L < 32 || L > 256 || L % 32) throw std::invalid_argument(w + ": latent must be a multiple of 32 in 32 .. 256");
  if (W_lat->rows != (size_t)H || W_lat->cols != 2 * L) throw std::invalid_argument(w + ": W_lat must be hidden x (2 latent)");
  if (b_lat->rows != 1 || b_lat->cols != 2 * L) throw std::invalid_argument(w + ": b_lat must be 1 x (2 latent)");
  if (W_dec->cols != (size_t)H) throw std::invalid_argument(w + ": W_dec must be latent x hidden");
  if (b_dec->rows != 1 || b_dec->cols != (size_t)H) throw std::invalid_argument(w + ": b_dec must be 1 x hidden");
  return (int)L;
}

void launch_forward(const Batch &b, int L, const VaeParams &p, int sample, const float *h1, float *mu_lv, float *eps, float *z,
                    float *kl_part, float *out, int ld, float *h2T, float *kl) {
  const int row_blocks = (b.B + kTile - 1) / kTile;
  IMP_PROF("vae_forward");
  vae_latent_kernel<<<row_blocks * (L / 32), 256, 0, stream()>>>(Latent{b, h1, p.W_lat, p.b_lat, L, sample, mu_lv, eps, z, kl_part});
  vae_hidden_kernel<<<row_blocks * ((b.H + kTile - 1) / kTile), 256, 0, stream()>>>(Hidden{z, p.W_dec, p.b_dec, b.B, L, b.H, out, ld, h2T, kl_part, kl});
  IMP_CHECK_HIP(hipGetLastError());
}

struct VaeGradients {
  float *dW_in, *db_in, *dW_lat, *db_lat, *dW_dec, *db_dec, *dW_out;  // dW_in NULL: all taken from the workspace (imp_vae_step)
  float *mu_lv, *eps, *dh2;
};
// What a queued batch leaves on the device: three words (NLL, the encoder's unsorted flag, KL) and the gradients.
struct VaeQueued {
  const float *words;
  VaeGradients g;
};

VaeQueued queue_vae(const imp_csr *C, const int32_t *rows, int B, int H, int L, const VaeParams &p, float dropout, uint64_t seed,
                    float beta, int sample, VaeGradients g) {
  const int items = C->cols, tiles = (items + kTile - 1) / kTile;
  const int grid = std::min(tiles, std::max(1, ctx().num_cus));
  const size_t bh = (size_t)B * H, bl = (size_t)B * L, stats_n = round64(3 * (size_t)tiles * B);
  const size_t n_in = (size_t)items * H, n_out = (size_t)items * (H + 1), n_lat = (size_t)H * 2 * L, n_dec = (size_t)L * H;
  const bool own = !g.dW_in;
  const size_t own_n = round64(n_in) + 2 * round64(H) + round64(n_lat) + round64(2 * L) + round64(n_dec) + round64(n_out) + 3 * bl + bh;
  const size_t need = round64(B) + 5 * bh + stats_n + 2 * round64(B) + 64 + (size_t)grid * bh + 3 * bl + (size_t)(L / 32) * B + (own ? own_n : 0);
  float *ws = ctx().dae_ws.reserve(need);
  int32_t *rows_d = reinterpret_cast<int32_t *>(ws);
  float *h1 = ws + round64(B), *h2 = h1 + bh, *h2T = h2 + bh, *dz2 = h2T + bh, *dz1 = dz2 + bh, *stats = dz1 + bh;
  float *lse = stats + stats_n, *row_loss = lse + round64(B), *words = row_loss + round64(B), *partial = words + 64;
  float *z = partial + (size_t)grid * bh, *da = z + bl, *kl_part = da + 2 * bl;
  if (own) {
    float *q = kl_part + (size_t)(L / 32) * B;
    g.dW_in = q, q += round64(n_in);
    g.db_in = q, q += round64(H);
    g.dW_lat = q, q += round64(n_lat);
    g.db_lat = q, q += round64(2 * L);
    g.dW_dec = q, q += round64(n_dec);
    g.db_dec = q, q += round64(H);
    g.dW_out = q, q += round64(n_out);
    g.mu_lv = q, q += 2 * bl;
    g.eps = q, q += bl;
    g.dh2 = q;
  }
  int *unsorted = reinterpret_cast<int *>(words + 1);
  IMP_CHECK_HIP(hipMemcpyAsync(rows_d, rows, (size_t)B * 4, hipMemcpyHostToDevice, stream()));
  IMP_CHECK_HIP(hipMemsetAsync(words, 0, 64 * 4, stream()));
  const Batch b{C->indptr.data(), C->indices.data(), rows_d, B, H, items, dropout, seed};
  {
    IMP_PROF("vae_encode");
    dae_zero_kernel<<<(unsigned)std::min<size_t>((n_in + 255) / 256, (size_t)ctx().num_cus * 8), 256, 0, stream()>>>(g.dW_in, n_in);
    dae_encode_kernel<<<B, 256, 0, stream()>>>(b, p.W_in, p.b_in, h1, H, nullptr, unsorted);
    IMP_CHECK_HIP(hipGetLastError());
  }
  launch_forward(b, L, p, sample, h1, g.mu_lv, g.eps, z, kl_part, h2, H, h2T, words + 2);
  const Decode d{b, p.W_out, h2, h2T, stats, lse, g.dW_out, partial, tiles};
  const size_t lds = decode_lds_bytes(H);
  {
    IMP_PROF("vae_pass1");
    allow_dynamic_lds(dae_decode_kernel<1, 1>, lds);
    dae_decode_kernel<1, 1><<<grid, 256, lds, stream()>>>(d);
    dae_merge_kernel<<<(B + 3) / 4, 256, 0, stream()>>>(b, stats, tiles, lse, row_loss);
    IMP_CHECK_HIP(hipGetLastError());
  }
  {
    IMP_PROF("vae_pass2");
    auto launch = [&](auto kernel) {
      allow_dynamic_lds(kernel, lds);
      kernel<<<grid, 256, lds, stream()>>>(d);
    };
    switch ((H + 63) / 64) {
      case 1: launch(dae_decode_kernel<2, 1>); break;
      case 2: launch(dae_decode_kernel<2, 2>); break;
      case 3:
      case 4: launch(dae_decode_kernel<2, 4>); break;
      default: launch(dae_decode_kernel<2, 8>); break;
    }
    dae_fold_kernel<<<(unsigned)((bh + 255) / 256), 256, 0, stream()>>>(partial, grid, bh, h2, g.dh2, dz2);
    IMP_CHECK_HIP(hipGetLastError());
  }
  {
    IMP_PROF("vae_backward");
    launch_backward<1>(Backward{b, dz2, p.W_dec, z, H, L, g.dW_dec, g.db_dec, da, g.mu_lv, g.eps, beta / (float)B});
    launch_backward<2>(Backward{b, da, p.W_lat, h1, 2 * L, H, g.dW_lat, g.db_lat, dz1, nullptr, nullptr, 0.f});
    IMP_CHECK_HIP(hipGetLastError());
  }
  {
    IMP_PROF("vae_rest");
    dae_bias_loss_kernel<<<(H + 255) / 256 + 1, 256, 0, stream()>>>(dz1, B, H, g.db_in, row_loss, words);
    dae_scatter_kernel<<<B, 256, 0, stream()>>>(b, dz1, g.dW_in);
    IMP_CHECK_HIP(hipGetLastError());
  }
  return {words, g};
}

// waits for the stream; NLL and KL, or invalid_argument when the encoder met a row that is not strictly ascending
void finish_vae(const std::string &w, const VaeQueued &q, float *nll, float *kl) {
  float host[3];
  IMP_CHECK_HIP(hipMemcpyAsync(host, q.words, sizeof(host), hipMemcpyDeviceToHost, stream()));
  sync();
  int flag;
  memcpy(&flag, host + 1, sizeof(flag));
  if (flag) throw std::invalid_argument(w + ": a row of user_items is not strictly ascending (sort_indices / sum_duplicates first)");
  *nll = host[0], *kl = host[2];
}

void no_overlap(const std::string &w, const imp_matrix *const *all, int n) {
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < i; ++j)
      if (all[i]->overlaps(all[j])) throw std::invalid_argument(w + ": two of the matrices share storage");
}

}  // namespace
}  // namespace imp

using namespace imp;

extern "C" int imp_vae_encode(const imp_csr *user_items, const int32_t *rows, int64_t n_rows, const imp_matrix *W_in,
                              const imp_matrix *b_in, const imp_matrix *W_lat, const imp_matrix *b_lat, const imp_matrix *W_dec,
                              const imp_matrix *b_dec, imp_matrix *out) {
  return guarded([&] {
    const std::string w("vae_encode");
    if (!user_items || !W_in || !b_in || !W_lat || !b_lat || !W_dec || !b_dec || !out) throw std::invalid_argument(w + ": NULL argument");
    const int H = hidden_of(w, user_items, W_in, b_in, nullptr);
    const int L = latent_of(w, H, W_lat, b_lat, W_dec, b_dec);
    if (n_rows < 0 || n_rows > INT32_MAX) throw std::invalid_argument(w + ": bad row count");
    if (out->itemsize != 4 || out->rows != (size_t)n_rows || out->cols != (size_t)H + 1) throw std::invalid_argument(w + ": out must be float32, rows x (hidden + 1)");
    const imp_matrix *all[] = {W_in, b_in, W_lat, b_lat, W_dec, b_dec, out};
    for (int i = 0; i < 6; ++i)
      if (out->overlaps(all[i])) throw std::invalid_argument(w + ": out shares storage with a parameter");
    check_rows(w, user_items, rows, n_rows);
    if (n_rows == 0) return;
    const size_t n = (size_t)n_rows, nl = n * L;
    float *ws = ctx().dae_ws.reserve(round64(n) + 64 + round64(n * H) + 4 * round64(nl) + (size_t)(L / 32) * n);
    int32_t *rows_d = reinterpret_cast<int32_t *>(ws);
    int *unsorted = reinterpret_cast<int *>(ws + round64(n));
    float *h1 = ws + round64(n) + 64, *mu_lv = h1 + round64(n * H), *eps = mu_lv + 2 * round64(nl), *z = eps + round64(nl), *kl_part = z + round64(nl);
    IMP_CHECK_HIP(hipMemcpyAsync(rows_d, rows, n * 4, hipMemcpyHostToDevice, stream()));
    IMP_CHECK_HIP(hipMemsetAsync(unsorted, 0, 4, stream()));
    const Batch b{user_items->indptr.data(), user_items->indices.data(), rows_d, (int)n_rows, H, user_items->cols, 0.f, 0};
    {
      IMP_PROF("vae_encode");
      dae_encode_kernel<<<(unsigned)n_rows, 256, 0, stream()>>>(b, W_in->f32(), b_in->f32(), h1, H, nullptr, unsorted);
      IMP_CHECK_HIP(hipGetLastError());
    }
    const VaeParams p{W_in->f32(), b_in->f32(), W_lat->f32(), b_lat->f32(), W_dec->f32(), b_dec->f32(), nullptr};
    launch_forward(b, L, p, 0, h1, mu_lv, eps, z, kl_part, out->mut<float>(), H + 1, nullptr, nullptr);
    int flag = 0;
    IMP_CHECK_HIP(hipMemcpyAsync(&flag, unsorted, 4, hipMemcpyDeviceToHost, stream()));
    sync();  // the row ids are the caller's memory
    if (flag) throw std::invalid_argument(w + ": a row of user_items is not strictly ascending (sort_indices / sum_duplicates first)");
  });
}

extern "C" int imp_vae_gradients(const imp_csr *user_items, const int32_t *rows, int64_t batch_size, const imp_matrix *W_in,
                                 const imp_matrix *b_in, const imp_matrix *W_lat, const imp_matrix *b_lat, const imp_matrix *W_dec,
                                 const imp_matrix *b_dec, const imp_matrix *W_out, float dropout, int64_t seed, float beta, int sample,
                                 imp_matrix *dW_in, imp_matrix *db_in, imp_matrix *dW_lat, imp_matrix *db_lat, imp_matrix *dW_dec,
                                 imp_matrix *db_dec, imp_matrix *dW_out, imp_matrix *mu_lv, imp_matrix *eps, imp_matrix *dh2, float *nll,
                                 float *kl) {
  return guarded([&] {
    const std::string w("vae_gradients");
    if (!user_items || !W_in || !b_in || !W_lat || !b_lat || !W_dec || !b_dec || !W_out || !nll || !kl) throw std::invalid_argument(w + ": NULL argument");
    const int H = hidden_of(w, user_items, W_in, b_in, W_out);
    const int L = latent_of(w, H, W_lat, b_lat, W_dec, b_dec);
    check_batch(w, batch_size, dropout);
    if (!(beta >= 0.f)) throw std::invalid_argument(w + ": beta must not be negative");
    same_shape(w, dW_in, W_in, "dW_in"), same_shape(w, db_in, b_in, "db_in"), same_shape(w, dW_lat, W_lat, "dW_lat");
    same_shape(w, db_lat, b_lat, "db_lat"), same_shape(w, dW_dec, W_dec, "dW_dec"), same_shape(w, db_dec, b_dec, "db_dec");
    same_shape(w, dW_out, W_out, "dW_out");
    const size_t B = (size_t)batch_size;
    auto shaped = [&](const imp_matrix *m, size_t cols) { return m && m->itemsize == 4 && m->rows == B && m->cols == cols; };
    if (!shaped(mu_lv, 2 * (size_t)L) || !shaped(eps, L) || !shaped(dh2, H))
      throw std::invalid_argument(w + ": mu_lv, eps, dh2 must be float32, batch_size x (2 latent), latent, hidden");
    const imp_matrix *all[] = {W_in, b_in, W_lat, b_lat, W_dec, b_dec, W_out, dW_in, db_in, dW_lat, db_lat, dW_dec, db_dec, dW_out, mu_lv, eps, dh2};
    no_overlap(w, all, 17);
    check_rows(w, user_items, rows, batch_size);
    const VaeParams p{W_in->f32(), b_in->f32(), W_lat->f32(), b_lat->f32(), W_dec->f32(), b_dec->f32(), W_out->f32()};
    const VaeGradients g{dW_in->mut<float>(), db_in->mut<float>(), dW_lat->mut<float>(), db_lat->mut<float>(), dW_dec->mut<float>(),
                         db_dec->mut<float>(), dW_out->mut<float>(), mu_lv->mut<float>(), eps->mut<float>(), dh2->mut<float>()};
    finish_vae(w, queue_vae(user_items, rows, (int)batch_size, H, L, p, dropout, (uint64_t)seed, beta, sample != 0, g), nll, kl);
  });
}

extern "C" int imp_vae_step(const imp_csr *user_items, const int32_t *rows, int64_t batch_size, imp_matrix *const *params,
                            imp_matrix *const *moments, float dropout, int64_t seed, float beta, float learning_rate, float beta1,
                            float beta2, float eps, float regularization, int64_t step, float *nll, float *kl) {
  return guarded([&] {
    const std::string w("vae_step");
    if (!user_items || !params || !moments || !nll || !kl) throw std::invalid_argument(w + ": NULL argument");
    const imp_matrix *all[21];
    for (int i = 0; i < 7; ++i) all[i] = params[i];
    for (int i = 0; i < 14; ++i) all[7 + i] = moments[i];
    for (const imp_matrix *m : all)
      if (!m) throw std::invalid_argument(w + ": NULL argument");
    const int H = hidden_of(w, user_items, params[0], params[1], params[6]);
    const int L = latent_of(w, H, params[2], params[3], params[4], params[5]);
    check_batch(w, batch_size, dropout);
    if (!(beta >= 0.f)) throw std::invalid_argument(w + ": beta must not be negative");
    if (step < 1) throw std::invalid_argument(w + ": step counts from 1");
    if (!(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps > 0.f)) throw std::invalid_argument(w + ": beta1, beta2 must lie in [0, 1) and eps above 0");
    for (int i = 0; i < 14; ++i) same_shape(w, moments[i], params[i / 2], "a moment matrix");
    no_overlap(w, all, 21);
    check_rows(w, user_items, rows, batch_size);
    const VaeParams p{params[0]->f32(), params[1]->f32(), params[2]->f32(), params[3]->f32(), params[4]->f32(), params[5]->f32(), params[6]->f32()};
    const VaeQueued q = queue_vae(user_items, rows, (int)batch_size, H, L, p, dropout, (uint64_t)seed, beta, 1, VaeGradients{});
    {
      IMP_PROF("vae_adam");
      const float *grads[7] = {q.g.dW_in, q.g.db_in, q.g.dW_lat, q.g.db_lat, q.g.dW_dec, q.g.db_dec, q.g.dW_out};
      const int ld[7] = {H, H, 2 * L, 2 * L, H, H, H + 1}, decay[7] = {H, 0, 2 * L, 0, H, 0, H};
      AdamArgs a{};
      a.lr = learning_rate, a.b1 = beta1, a.b2 = beta2, a.eps = eps, a.reg = regularization;
      a.c1 = (float)(1.0 / (1.0 - std::pow((double)beta1, (double)step)));
      a.c2 = (float)(1.0 / (1.0 - std::pow((double)beta2, (double)step)));
      a.unsorted = reinterpret_cast<const int *>(q.words + 1);
      for (int first = 0; first < 7; first += 3) {  // Mult-DAE's kernel takes three segments a launch
        size_t longest = 1;
        for (int s = 0; s < 3; ++s) {
          const int i = first + s;
          a.seg[s] = AdamSegment{};
          if (i >= 7) continue;
          const size_t n = params[i]->rows * params[i]->cols;
          a.seg[s] = {params[i]->mut<float>(), moments[2 * i]->mut<float>(), moments[2 * i + 1]->mut<float>(), grads[i], n, ld[i], decay[i]};
          longest = std::max(longest, n);
        }
        dae_adam_kernel<<<(unsigned)std::min<size_t>((longest + 255) / 256, (size_t)ctx().num_cus * 8), 256, 0, stream()>>>(a);
      }
      IMP_CHECK_HIP(hipGetLastError());
    }
    finish_vae(w, q, nll, kl);
  });
}
