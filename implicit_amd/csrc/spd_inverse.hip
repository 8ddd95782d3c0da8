// K16a: in-place inverse of a dense symmetric positive definite fp32 matrix (imp_spd_inverse) -- the fit of EASE.
//
// Blocked Cholesky inverse, block size nb = kSpdBlock (128; 64 measured slower).  Every dependency between
// steps is a kernel boundary on the library stream: no spin-waits, no tickets, no persistent workgroups.  With A = L L^T and
// V = L^-T (upper triangular), A^-1 = V V^T.  Only the lower triangle of A is read.
//   phase 1, factor (right-looking), for every block column k:
//     spd_diag_kernel   one workgroup: A_kk = L_kk L_kk^T in registers (a 16 x 16 cyclic deal of the block, the pivot column
//                       published through the LDS) and W_kk = L_kk^-1 in the LDS (forward substitution on the two half blocks,
//                       one thread per column, the off-diagonal quarter as two small products); L_kk goes back into A, W_kk to a side array, W_kk^T into V's diagonal block
//     panel             L_ik = A_ik W_kk^T   (i > k), in place: one workgroup owns a whole row stripe of the panel
//     trailing update   A_ij -= L_ik L_jk^T  (i >= j > k, lower tiles only)
//   phase 2, V = L^-T block column by block column, from V L^T = I:  V_ik = -(sum_{i <= j < k} V_ij L_kj^T) W_kk^T  (i < k),
//     right-looking as well: V starts zeroed; once block column k is final (its sums times -W_kk^T, in place), the products
//     V_ik L_jk^T are added to the sums of every block column j > k in one launch over all of them.
//   phase 3, P = V V^T over the lower tiles (the sum starts at the tile's first row: V is zero left of its diagonal), written
//     over A, then mirror_lower copies the lower triangle into the upper one: the result is exactly symmetric.
// All the products are the ONE building block gemm_nt_kernel: C = alpha A B^T + beta C on 128 x 128 x 16 tiles, operands
// staged through the LDS, 2 x 2 tiles of v_mfma_f32_32x32x2_f32 per wavefront (exact fp32 products and sums in a fixed order:
// equal inputs give bitwise equal outputs).  Ragged edges (n not a multiple of nb or of the tile) are masked: rows and columns
// outside a matrix load as zeros and are never stored; the padded part of a diagonal block is the identity.
// A non-positive or NaN pivot stores its index with atomicMin in a device word; every later kernel reads the word first and
// returns at once, so a failed call ends promptly without a host round trip per step.
// Workspace: V (n x n) + the W_kk (n x nb, rounded up).
#include <type_traits>

#include "common.h"
#include "spd_inverse.h"

namespace imp {

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {
constexpr int kGemmTile = 128, kGemmK = 16, kGemmLd = kGemmK + 1;
constexpr int kSpdBlock = 128;  // at most kGemmTile: the in-place panel product relies on one column of tiles

struct GemmArgs {
  const float *A;  // a_rows x (>= k_end), row stride lda
  long lda;
  int a_rows;
  const float *B;  // b_rows x (>= k_end), row stride ldb
  long ldb;
  int b_rows;
  float *C;  // a_rows x b_rows, row stride ldc; may alias A when a single column of tiles is launched (the panel)
  long ldc;
  int k_begin, k_end;  // the columns of A and B that are contracted
  int tri_k;           // the sum starts at the tile's first row (A is zero left of its diagonal)
  int lower_only;      // tiles above the diagonal are skipped
  float alpha, beta;   // C = alpha A B^T + beta C; beta == 0 never reads C
  const unsigned long long *failed;
};

__global__ __launch_bounds__(256) void gemm_nt_kernel(GemmArgs g) {
  __shared__ float As[kGemmTile * kGemmLd], Bs[kGemmTile * kGemmLd];
  if (*g.failed != kNoFailure) return;
  const int row0 = blockIdx.y * kGemmTile, col0 = blockIdx.x * kGemmTile;
  if (g.lower_only && col0 > row0) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int kcol = tid & 15, rbase = tid >> 4;
  float ra[8], rb[8];
  auto fetch = [&](int kk) {
    const int p = kk + kcol;
    const bool pk = p < g.k_end;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = rbase + 16 * i;
      ra[i] = (pk && row0 + r < g.a_rows) ? g.A[(long)(row0 + r) * g.lda + p] : 0.f;
      rb[i] = (pk && col0 + r < g.b_rows) ? g.B[(long)(col0 + r) * g.ldb + p] : 0.f;
    }
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 2; ++nj)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[mi][nj][e] = 0.f;
  int k = g.tri_k ? max(g.k_begin, row0) : g.k_begin;
  if (k < g.k_end) fetch(k);
  const int a_off = (wm * 64 + (lane & 31)) * kGemmLd + (lane >> 5);
  const int b_off = (wn * 64 + (lane & 31)) * kGemmLd + (lane >> 5);
  for (; k < g.k_end; k += kGemmK) {
    __syncthreads();  // the previous chunk has been consumed
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      As[(rbase + 16 * i) * kGemmLd + kcol] = ra[i];
      Bs[(rbase + 16 * i) * kGemmLd + kcol] = rb[i];
    }
    __syncthreads();
    if (k + kGemmK < g.k_end) fetch(k + kGemmK);  // in flight during the products below
#pragma unroll
    for (int ks = 0; ks < kGemmK / 2; ++ks) {
      const float a0 = As[a_off + 2 * ks], a1 = As[a_off + 32 * kGemmLd + 2 * ks];
      const float b0 = Bs[b_off + 2 * ks], b1 = Bs[b_off + 32 * kGemmLd + 2 * ks];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
  // C/D layout of a 32 x 32 tile: col = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 2; ++nj) {
      const int c = col0 + wn * 64 + nj * 32 + (lane & 31);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int r = row0 + wm * 64 + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        if (r < g.a_rows && c < g.b_rows) {
          float *dst = g.C + (long)r * g.ldc + c;
          const float v = g.alpha * acc[mi][nj][e];
          *dst = g.beta != 0.f ? g.beta * *dst + v : v;
        }
      }
    }
}

template <int N, int I = 0, typename Fn> __device__ __forceinline__ bool static_all(Fn &&fn) {
  if constexpr (I < N) {
    if (!fn(std::integral_constant<int, I>{})) return false;
    return static_all<N, I + 1>(fn);
  }
  return true;
}

// One workgroup: the diagonal block at index k0 (m = min(NB, n - k0) rows; the padding is the identity).
template <int NB>
__global__ __launch_bounds__(256) void spd_diag_kernel(float *A, long n, int k0, float *__restrict__ Wd, float *__restrict__ V,
                                                       unsigned long long *failed) {
  extern __shared__ float spd_lds[];
  constexpr int LD = NB + 1;
  float *L = spd_lds, *W = spd_lds + NB * LD;
  if (*failed != kNoFailure) return;
  __shared__ float col[NB];
  __shared__ float pivot;
  const int tid = threadIdx.x;
  const int m = (int)min((long)NB, n - k0);
  // Factor: thread (ty, tx) keeps the elements (ty + 16 p, tx + 16 q) in registers for the whole factorisation (a cyclic deal:
  // the load stays even as the columns retire).  Column j is published through the LDS by the 16 threads that own it.
  constexpr int T = NB / 16;
  const int tx = tid & 15, ty = tid >> 4;
  float a[T][T];
#pragma unroll
  for (int p = 0; p < T; ++p)
#pragma unroll
    for (int q = 0; q < T; ++q) {
      const int r = ty + 16 * p, c = tx + 16 * q;
      a[p][q] = (r < m && c <= r) ? A[(long)(k0 + r) * n + k0 + c] : (r == c ? 1.f : 0.f);
    }
  // (the block column jq of the pivot is a compile-time constant: every register of `a` is addressed by name)
  const bool ok = static_all<T>([&](auto jq_c) {
    constexpr int jq = decltype(jq_c)::value;
    for (int jj = 0; jj < 16; ++jj) {
      const int j = 16 * jq + jj;
      if (j >= m) break;  // the padding is the identity already
      if (ty == jj && tx == jj) pivot = a[jq][jq];
      __syncthreads();
      const float d = pivot;
      if (!(d > 0.f)) {  // the same value in every thread: the workgroup leaves together
        if (tid == 0) atomicMin(failed, (unsigned long long)(k0 + j));
        return false;
      }
      const float s = sqrtf(d);
      if (tx == jj) {
#pragma unroll
        for (int p = jq; p < T; ++p) {
          const int r = ty + 16 * p;
          if (r >= j) a[p][jq] = r == j ? s : a[p][jq] / s;
          col[r] = a[p][jq];
        }
      }
      __syncthreads();
      float lr[T], lc[T];
#pragma unroll
      for (int p = jq; p < T; ++p) lr[p] = col[ty + 16 * p], lc[p] = col[tx + 16 * p];
#pragma unroll
      for (int p = jq; p < T; ++p)
#pragma unroll
        for (int q = jq; q < T; ++q) {
          const int r = ty + 16 * p, c = tx + 16 * q;
          if (c > j && c <= r) a[p][q] -= lr[p] * lc[q];
        }
    }
    return true;
  });
  if (!ok) return;
#pragma unroll
  for (int p = 0; p < T; ++p)
#pragma unroll
    for (int q = 0; q < T; ++q) L[(ty + 16 * p) * LD + tx + 16 * q] = a[p][q];
  __syncthreads();
  // W = L^-1 in halves, L = [L11 0; L21 L22]: W11 and W22 by forward substitution (thread c owns column c of its half and reads
  // back only what it wrote itself; four partial sums keep four LDS round trips in flight), then W21 = -W22 (L21 W11) as two
  // small products by the whole workgroup, the first one parked in the (zero) upper right block of W
  constexpr int H = NB / 2;
  if (tid < NB) {
    const int c = tid, i0 = c < H ? 0 : H, i1 = i0 + H;
    for (int i = i0; i < i1; ++i) {
      float s0 = i == c ? 1.f : 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
      int j = c;
      for (; j + 3 < i; j += 4) {
        s0 -= L[i * LD + j] * W[j * LD + c];
        s1 -= L[i * LD + j + 1] * W[(j + 1) * LD + c];
        s2 -= L[i * LD + j + 2] * W[(j + 2) * LD + c];
        s3 -= L[i * LD + j + 3] * W[(j + 3) * LD + c];
      }
      for (; j < i; ++j) s0 -= L[i * LD + j] * W[j * LD + c];
      W[i * LD + c] = i < c ? 0.f : ((s0 + s1) + (s2 + s3)) / L[i * LD + i];
    }
  }
  __syncthreads();
  constexpr int E = H / 16;  // thread (ty, tx) computes the E x E entries (ty + 16 p, tx + 16 q) of a product of halves
  {
    float t1[E][E];
#pragma unroll
    for (int p = 0; p < E; ++p)
#pragma unroll
      for (int q = 0; q < E; ++q) t1[p][q] = 0.f;
    for (int k = 0; k < H; ++k) {
      float l[E], w[E];
#pragma unroll
      for (int p = 0; p < E; ++p) l[p] = L[(H + ty + 16 * p) * LD + k], w[p] = W[k * LD + tx + 16 * p];
#pragma unroll
      for (int p = 0; p < E; ++p)
#pragma unroll
        for (int q = 0; q < E; ++q) t1[p][q] += l[p] * w[q];
    }
#pragma unroll
    for (int p = 0; p < E; ++p)
#pragma unroll
      for (int q = 0; q < E; ++q) W[(ty + 16 * p) * LD + H + tx + 16 * q] = t1[p][q];
  }
  __syncthreads();
  {
    float t2[E][E];
#pragma unroll
    for (int p = 0; p < E; ++p)
#pragma unroll
      for (int q = 0; q < E; ++q) t2[p][q] = 0.f;
    for (int k = 0; k < H; ++k) {
      float l[E], w[E];
#pragma unroll
      for (int p = 0; p < E; ++p) l[p] = W[(H + ty + 16 * p) * LD + H + k], w[p] = W[k * LD + H + tx + 16 * p];
#pragma unroll
      for (int p = 0; p < E; ++p)
#pragma unroll
        for (int q = 0; q < E; ++q) t2[p][q] -= l[p] * w[q];
    }
    __syncthreads();  // the parked product has been read
#pragma unroll
    for (int p = 0; p < E; ++p)
#pragma unroll
      for (int q = 0; q < E; ++q) {
        W[(H + ty + 16 * p) * LD + tx + 16 * q] = t2[p][q];
        W[(ty + 16 * p) * LD + H + tx + 16 * q] = 0.f;
      }
  }
  __syncthreads();
  for (int t = tid; t < NB * NB; t += 256) {
    const int r = t / NB, c = t % NB;
    Wd[t] = W[r * LD + c];
    if (r < m && c < m) {
      if (c <= r) A[(long)(k0 + r) * n + k0 + c] = L[r * LD + c];
      V[(long)(k0 + r) * n + k0 + c] = W[c * LD + r];
    }
  }
}

__global__ __launch_bounds__(256) void mirror_lower_kernel(float *A, long n) {
  __shared__ float tile[32][33];
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj > bi) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const long r = (long)bi * 32 + ty + 8 * q, c = (long)bj * 32 + tx;
    if (r < n && c < n) tile[ty + 8 * q][tx] = A[r * n + c];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const long r = (long)bj * 32 + ty + 8 * q, c = (long)bi * 32 + tx;  // (r, c) above the diagonal takes (c, r)
    if (r < n && c < n && r < c) A[r * n + c] = tile[tx][ty + 8 * q];
  }
}

void launch_gemm(const GemmArgs &g) {
  const unsigned tn = (unsigned)((g.b_rows + kGemmTile - 1) / kGemmTile), tm = (unsigned)((g.a_rows + kGemmTile - 1) / kGemmTile);
  if (tn == 0 || tm == 0) return;
  gemm_nt_kernel<<<dim3(tn, tm), 256, 0, stream()>>>(g);
  IMP_CHECK_HIP(hipGetLastError());
}

template <int NB> void launch_diag(float *A, long n, int k0, float *Wd, float *V, unsigned long long *failed) {
  constexpr size_t lds = 2 * (size_t)NB * (NB + 1) * sizeof(float);
  allow_dynamic_lds_once<spd_diag_kernel<NB>>(lds);
  spd_diag_kernel<NB><<<1, 256, lds, stream()>>>(A, n, k0, Wd, V, failed);
  IMP_CHECK_HIP(hipGetLastError());
}

}  // namespace

void mirror_lower(float *A, size_t n) {
  if (n < 2) return;
  const unsigned t = (unsigned)((n + 31) / 32);
  mirror_lower_kernel<<<dim3(t, t), 256, 0, stream()>>>(A, (long)n);
  IMP_CHECK_HIP(hipGetLastError());
}

// -1, or the smallest failing pivot
static int64_t spd_inverse(float *A, size_t n_) {
  const long n = (long)n_;
  constexpr int nb = kSpdBlock;
  const int nblk = (int)((n + nb - 1) / nb);
  const size_t need = ((size_t)n * n + (size_t)nblk * nb * nb) * sizeof(float);
  DeviceArray<float> ws;
  try {
    ws.alloc((size_t)n * n + (size_t)nblk * nb * nb);
  } catch (const std::exception &e) {
    throw std::runtime_error("spd_inverse: cannot allocate the workspace of " + std::to_string(need) + " bytes for n = " +
                             std::to_string(n) + " (" + e.what() + ")");
  }
  float *V = ws.data(), *Wd = V + (size_t)n * n;
  unsigned long long *failed = reset_fail_word();
  IMP_CHECK_HIP(hipMemsetAsync(V, 0, (size_t)n * n * sizeof(float), stream()));
  {
    IMP_PROF_NESTED("spd_inverse_factor");
    for (int k = 0; k < nblk; ++k) {
      const int k0 = k * nb;
      float *Wk = Wd + (size_t)k * nb * nb;
      launch_diag<nb>(A, n, k0, Wk, V, failed);
      const int rem = (int)(n - (k0 + nb));
      if (rem <= 0) break;
      float *Ak = A + (size_t)(k0 + nb) * n + k0;  // the panel below the diagonal block
      launch_gemm(GemmArgs{Ak, n, rem, Wk, nb, nb, Ak, n, 0, nb, 0, 0, 1.f, 0.f, failed});
      launch_gemm(GemmArgs{Ak, n, rem, Ak, n, rem, Ak + nb, n, 0, nb, 0, 1, -1.f, 1.f, failed});
    }
  }
  {
    IMP_PROF_NESTED("spd_inverse_tri");
    for (int k = 0; k < nblk; ++k) {
      const int k0 = k * nb, kb = (int)std::min<long>(nb, n - k0);
      float *Wk = Wd + (size_t)k * nb * nb;
      // block column k of V above its diagonal block holds S = sum_j V_ij L_kj^T: V_ik = -S W_kk^T, in place
      launch_gemm(GemmArgs{V + k0, n, k0, Wk, nb, kb, V + k0, n, 0, kb, 0, 0, -1.f, 0.f, failed});
      const int rem = (int)(n - (k0 + nb));
      if (rem <= 0) break;
      // the finished block column goes into the sums of every block column to its right
      launch_gemm(GemmArgs{V + k0, n, k0 + nb, A + (size_t)(k0 + nb) * n + k0, n, rem, V + k0 + nb, n, 0, nb, 0, 0, 1.f, 1.f, failed});
    }
  }
  {
    IMP_PROF_NESTED("spd_inverse_wtw");
    launch_gemm(GemmArgs{V, n, (int)n, V, n, (int)n, A, n, 0, (int)n, 1, 1, 1.f, 0.f, failed});
    mirror_lower(A, (size_t)n);
  }
  return read_fail_word(failed);
}

}  // namespace imp

using namespace imp;

extern "C" int imp_spd_inverse(imp_matrix *A, int64_t *failed_pivot) {
  return guarded([&] {
    if (failed_pivot) *failed_pivot = -1;
    if (!A) throw std::invalid_argument("spd_inverse: NULL matrix");
    if (A->itemsize != 4 || A->rows != A->cols) throw std::invalid_argument("spd_inverse: the matrix must be square float32");
    if (A->rows > (size_t)INT32_MAX - 256) throw std::invalid_argument("spd_inverse: the order must stay below 2^31 - 256");
    if (A->rows == 0) return;
    IMP_PROF("spd_inverse");
    const int64_t failed = spd_inverse(A->mut<float>(), A->rows);
    if (failed >= 0) {
      if (failed_pivot) *failed_pivot = failed;
      throw std::invalid_argument("spd_inverse: the matrix is not positive definite (pivot " + std::to_string(failed) + " is not positive)");
    }
  });
}
