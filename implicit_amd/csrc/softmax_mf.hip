// K22: sampled-softmax matrix factorization -- one SGD epoch over mini-batches of 64 sampled positives, each batch against ONE
// set of N uniformly drawn negatives shared by its rows (imp_softmax_update).
//
// No reference counterpart: the listwise loss of Wu et al., "On the Effectiveness of Sampled Softmax Loss for Item
// Recommendation" (2022), with uniform negatives (so no logQ correction) and no temperature.  X (users x C) and Y (items x C)
// are float32 with C = factors + 1, 2 <= C <= 1024; column C-1 is the item bias, 1.0 in every user row and never written in X
// (as in bpr.hip and warp.hip; the kernel reads X[u,C-1] as the 1.0 it is).  userids / itemids are the COO ids of the CSR
// pattern, indptr its row pointers, row indices sorted; nnz < 2^31, items = Y.rows < 2^31.  N = `negatives` is a multiple of
// 32 in 32 .. 256.  Batch b of a call holds the samples s = 64 b + r, r = 0 .. 63, s < samples; the last batch may be partial
// and its missing rows contribute nothing.
//   1. positives: R = Philox4x32-10(counter (s_lo, s_hi, 0, 6), key (seed_lo, seed_hi)) (philox.h);  lp = (R.x * nnz) >> 32 in
//      64-bit arithmetic;  u_r = userids[lp], i_r = itemids[lp];
//   2. negatives: slot n = 0 .. N-1 takes word n & 3 of Philox(counter (b_lo, b_hi, 1 + (n >> 2), 6), same key) and
//      j_n = (word * items) >> 32 -- uniform over the items, shared by the 64 rows of the batch;
//   3. mask: M[r][n] = 1 when j_n is in row u_r of the pattern (j_n = i_r included).  A masked logit takes no part in row r's
//      softmax;
//   4. with every right-hand side read from BEFORE the batch's update:  z_r = X[u_r] . Y[i_r],  z_rn = X[u_r] . Y[j_n],
//      m_r = max over z_r and the unmasked z_rn,  p_r and p_rn = exp(. - m_r) over their sum, p_rn = 0 where masked.  A row
//      whose negatives are all masked has p_r = 1;
//   5. deltas, for the factor columns c < C-1:
//        dX[u_r,c] = lr ((1 - p_r) Y[i_r,c] - sum_n p_rn Y[j_n,c] - reg X[u_r,c])
//        dY[i_r,c] = lr ((1 - p_r) X[u_r,c] - reg Y[i_r,c])
//        dY[j_n,c] = lr (-sum_r p_rn X[u_r,c] - reg Y[j_n,c])      once per slot n, whether or not every row masks it
//      and for the bias column  dY[i_r,C-1] = lr ((1 - p_r) - reg Y[i_r,C-1]),  dY[j_n,C-1] = lr (-sum_r p_rn - reg Y[j_n,C-1]);
//   6. every delta of the batch is ADDED to its row: a user, a positive or a negative that occurs several times in a batch
//      receives the sum of its occurrences' deltas, a negative that is another row's positive included.
// The call returns (correct, masked): the rows with z_r > every unmasked z_rn, and sum M.
//
// Batches in flight: max(1, hogwild_in_flight(samples, users, items) / 64) workgroups (sgd_group.h: the family's cap on
// concurrent samples, in batches), each striding over the batches.  On a matrix with min(users, items) < 2048 that is ONE
// workgroup, and the call is then the serial mini-batch SGD stated above, batch after batch, up to fp32 rounding (the order of
// the sums); the tests rest on this.  With several workgroups the batches are Hogwild: a batch may read rows another batch
// is adding to, and the result is not reproducible (the counts neither).
//
// Kernel.  Not the lane-group layout of sgd_group.h: one workgroup of 256 threads (4 wavefronts) per batch, the batch's
// dependent chain three products long whatever N is.  The columns are cut into slices of 32; the LDS holds one slice of the
// user tile U (64 x 32), of the positives' tile Yp (64 x 32) and of the negatives' tile V (N x 32), leading dimension 33,
// and the whole P (64 x N), leading dimension N + 1: with the draws (98 N + 4608) x 4 bytes, 68 608 at N = 128 and
// 118 784 at N = 256.
//   draws    threads 0 .. 63 draw the positives and read their row bounds, threads 64 .. 64 + N/4 - 1 a Philox block of four
//            negatives each;
//   logits   per slice: 256 threads gather the three tiles (a row's 32 columns by 32 consecutive lanes), four threads per
//            row add the slice's part of z_r (row-wise dots, no matrix instruction), and the 64 x N logits accumulate in
//            2 N/32 tiles of v_mfma_f32_32x32x2_f32 -- exact fp32 products, the instruction of svd.hip and spd_inverse.hip --
//            up to 4 tiles per wavefront (TPW), all of a wavefront's tiles on one row block so that A is read once;
//   mask     one thread per (r, n), four threads per row: a branch-free binary search of the sorted row, eight searches
//            of a thread in lock step (one row, so one trip count) to keep eight loads in flight;
//   softmax  the same four threads: max, exp and sum by two shuffles, P left in the LDS (0 where masked);
//   deltas   the slices a second time: dY[i_r] element by element; wavefronts 0 and 1 form P V (their 32 rows x the slice,
//            K = N) and finish dX; wavefronts 2 and 3 form P^T U for the N/32 negative blocks (K = 64) and finish dY[j_n].
//            Both halves cost N matrix steps per slice.
// P's leading dimension N + 1 is odd.  P V reads P as A[row = lane & 31][k = lane >> 5]: the 32 lanes of a half-wavefront
// read one column of 32 rows, N + 1 words apart, which are 32 different banks because N + 1 is odd.  P^T U reads P as
// A[n = lane & 31][k = row = lane >> 5]: the 32 lanes read 32 consecutive words of one row.  So both operand orders read
// the one copy of P without a bank conflict inside a half-wavefront; the same holds for U, Yp and V with 33.
// Running the slices twice re-reads every gathered row once: 2 (128 + N) C floats per batch instead of (128 + N) C, from
// lines the first pass brought into the L2 a few microseconds earlier.  One slice width serves every C up to 1024, so the
// family's range costs nothing; nothing is compiled per C.
//
// Writes are agent-scope fp32 atomic adds (global_atomic_add_f32; _build.py passes -munsafe-fp-atomics so that they are
// not compare-and-swap loops), as step 6 demands, and for the reason DESIGN 4.15 measured for WARP's stores: a plain store stays in the writing XCD's L2, and a later kernel on another XCD reads an older
// row than a host copy holds.  Visibility between a workgroup's batches: after its last add every thread makes an
// agent-scope release fence (waits for its adds), the workgroup meets at a barrier, and the next batch opens with an
// agent-scope acquire fence (drops the CU's vector cache), so its gathers see the previous batch's adds.
//
// Every id the kernel turns into an address has been checked on the device first (check_pair_ids, pair_sgd.hip): an id
// outside its matrix returns IMP_OUT_OF_RANGE with nothing launched.  j_n < items by construction; the searches stay inside
// [indptr[u], indptr[u + 1]), which the pre-pass holds inside [0, nnz].
#include <string>

#include "common.h"
#include "philox.h"
#include "sgd_group.h"

namespace imp {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kRows = 64;        // positives per batch
constexpr int kSlice = 32;       // columns per slice
constexpr int kLd = kSlice + 1;  // leading dimension of U, Yp and V
constexpr int kSearches = 8;     // searches a thread runs in lock step

struct SoftmaxArgs {
  const int32_t *__restrict__ userids;
  const int32_t *__restrict__ itemids;
  const int32_t *__restrict__ indptr;
  float *X, *Y;  // rows are shared between concurrent batches: no __restrict__
  int64_t nnz, samples;
  uint64_t seed;
  float lr, reg;
  int C, items, N;
  unsigned long long *stats;  // [0] correct, [1] masked
};

size_t softmax_lds_bytes(int N) { return ((size_t)kRows * (N + 1) + 2 * kRows * kLd + (size_t)N * kLd + kRows + 4 * kRows + N) * 4; }

__device__ __forceinline__ void add_through(float *p, float v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// row of element e of a lane's 32 x 32 accumulator; its column is lane & 31
__device__ __forceinline__ int tile_row(int e, int lane) { return (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5); }

template <int TPW> __global__ __launch_bounds__(256) void softmax_update_kernel(SoftmaxArgs a) {
  extern __shared__ float lds[];
  const int N = a.N, C = a.C, ldp = N + 1;
  float *P = lds, *U = P + kRows * ldp, *Yp = U + kRows * kLd, *V = Yp + kRows * kLd, *gs = V + N * kLd;
  int *su = reinterpret_cast<int *>(gs + kRows), *si = su + kRows, *slo = si + kRows, *shi = slo + kRows, *sj = shi + kRows;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = tid & 31, slot = tid >> 5;  // the gathers: column of the slice, first row
  const int row = tid >> 2, q = tid & 3;      // the row-wise work: four threads per row
  const int l31 = lane & 31, lk = lane >> 5;  // the matrix operands
  const float lr = a.lr, reg = a.reg;
  const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
  const int64_t batches = (a.samples + kRows - 1) / kRows;
  unsigned long long correct = 0, masked = 0;

  auto gather = [&](int c0) {
    const int c = c0 + col;
    const bool in = c < C;
#pragma unroll
    for (int r = slot; r < kRows; r += 8) {
      const int u = su[r], i = si[r];
      U[r * kLd + col] = in && u >= 0 ? a.X[(size_t)u * C + c] : 0.f;
      Yp[r * kLd + col] = in && i >= 0 ? a.Y[(size_t)i * C + c] : 0.f;
    }
#pragma unroll 4
    for (int n = slot; n < N; n += 8) V[n * kLd + col] = in ? a.Y[(size_t)sj[n] * C + c] : 0.f;
  };

  for (int64_t b = blockIdx.x; b < batches; b += gridDim.x) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // the previous batch's adds, not the vector cache's lines
    const uint32_t b_lo = (uint32_t)b, b_hi = (uint32_t)((uint64_t)b >> 32);
    if (tid < kRows) {
      const int64_t s = b * kRows + tid;
      int u = -1, i = -1, lo = 0, hi = 0;
      if (s < a.samples) {
        const u32x4 r = philox4x32_10((uint32_t)s, (uint32_t)((uint64_t)s >> 32), 0u, 6u, k0, k1);
        const int64_t lp = (int64_t)(((uint64_t)r.x * (uint64_t)a.nnz) >> 32);
        u = a.userids[lp], i = a.itemids[lp];
        lo = a.indptr[u], hi = a.indptr[u + 1];
      }
      su[tid] = u, si[tid] = i, slo[tid] = lo, shi[tid] = hi;
    } else if (tid - kRows < N / 4) {
      const int g = tid - kRows;
      const u32x4 r = philox4x32_10(b_lo, b_hi, 1u + (uint32_t)g, 6u, k0, k1);
      const uint64_t items = (uint64_t)(uint32_t)a.items;
      sj[4 * g + 0] = (int)(((uint64_t)r.x * items) >> 32);
      sj[4 * g + 1] = (int)(((uint64_t)r.y * items) >> 32);
      sj[4 * g + 2] = (int)(((uint64_t)r.z * items) >> 32);
      sj[4 * g + 3] = (int)(((uint64_t)r.w * items) >> 32);
    }
    __syncthreads();

    // ---- logits: tile t = wave + 4 i is row block t & 1 = wave & 1, negative block t >> 1 = (wave >> 1) + 2 i
    f32x16 acc[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
    float z = 0.f;
    const int a_off = ((wave & 1) * 32 + l31) * kLd + lk;
    for (int c0 = 0; c0 < C; c0 += kSlice) {
      gather(c0);
      __syncthreads();
#pragma unroll
      for (int k = 0; k < kSlice / 4; ++k) z = fmaf(U[row * kLd + q + 4 * k], Yp[row * kLd + q + 4 * k], z);
#pragma unroll 4
      for (int ks = 0; ks < kSlice / 2; ++ks) {
        const float av = U[a_off + 2 * ks];
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
          const int nb = (wave >> 1) + 2 * i;
          if (nb * 32 < N) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, V[(nb * 32 + l31) * kLd + lk + 2 * ks], acc[i], 0, 0, 0);
        }
      }
      __syncthreads();  // the slice has been consumed
    }
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
      const int nb = (wave >> 1) + 2 * i;
      if (nb * 32 < N)
#pragma unroll
        for (int e = 0; e < 16; ++e) P[((wave & 1) * 32 + tile_row(e, lane)) * ldp + nb * 32 + l31] = acc[i][e];
    }
    z += __shfl_xor(z, 1);
    z += __shfl_xor(z, 2);  // z_r, the same in the row's four threads
    __syncthreads();

    // ---- mask and softmax: thread (row, q) owns the negatives n = q + 4 k
    {
      const bool valid = su[row] >= 0;
      const int lo = slo[row], hi = shi[row];
      float *Pr = P + row * ldp;
      float top = -INFINITY;  // the largest unmasked negative logit
      for (int g = 0; g < N / (4 * kSearches); ++g) {
        int j[kSearches], base[kSearches];
#pragma unroll
        for (int k = 0; k < kSearches; ++k) j[k] = sj[q + 4 * (kSearches * g + k)], base[k] = lo;
        int len = hi - lo;
        while (len > 1) {  // the last entry <= j lies in [base, base + len)
          const int half = len >> 1;
#pragma unroll
          for (int k = 0; k < kSearches; ++k) base[k] = a.itemids[base[k] + half] <= j[k] ? base[k] + half : base[k];
          len -= half;
        }
#pragma unroll
        for (int k = 0; k < kSearches; ++k) {
          const int n = q + 4 * (kSearches * g + k);
          if (len > 0 && a.itemids[base[k]] == j[k]) {
            Pr[n] = -INFINITY;
            ++masked;
          } else {
            top = fmaxf(top, Pr[n]);
          }
        }
      }
      top = fmaxf(top, __shfl_xor(top, 1));
      top = fmaxf(top, __shfl_xor(top, 2));
      const float m = fmaxf(top, z);
      float sum = 0.f;
      for (int n = q; n < N; n += 4) {
        const float e = expf(Pr[n] - m);  // 0 where masked
        Pr[n] = e;
        sum += e;
      }
      sum += __shfl_xor(sum, 1);
      sum += __shfl_xor(sum, 2);
      const float ez = expf(z - m);
      sum += ez;
      for (int n = q; n < N; n += 4) Pr[n] = valid ? Pr[n] / sum : 0.f;
      if (q == 0) {
        gs[row] = valid ? 1.f - ez / sum : 0.f;
        correct += valid && z > top;
      }
    }
    __syncthreads();

    // ---- deltas, slice by slice
    for (int c0 = 0; c0 < C; c0 += kSlice) {
      gather(c0);
      __syncthreads();
      if (c0 + col < C) {
#pragma unroll
        for (int r = slot; r < kRows; r += 8) {
          const int i = si[r];
          if (i >= 0) add_through(a.Y + (size_t)i * C + c0 + col, lr * (gs[r] * U[r * kLd + col] - reg * Yp[r * kLd + col]));
        }
      }
      const int c = c0 + l31;
      f32x16 d;
      if (wave < 2) {  // P V for the rows 32 wave .. + 31
#pragma unroll
        for (int e = 0; e < 16; ++e) d[e] = 0.f;
        const float *Pa = P + (wave * 32 + l31) * ldp + lk, *Vb = V + lk * kLd + l31;
#pragma unroll 8
        for (int n = 0; n < N; n += 2) d = __builtin_amdgcn_mfma_f32_32x32x2f32(Pa[n], Vb[n * kLd], d, 0, 0, 0);
        if (c < C - 1) {
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int r = wave * 32 + tile_row(e, lane), u = su[r];
            if (u >= 0) add_through(a.X + (size_t)u * C + c, lr * (gs[r] * Yp[r * kLd + l31] - d[e] - reg * U[r * kLd + l31]));
          }
        }
      } else {  // P^T U for the negative blocks wave - 2, wave, ...
        for (int nb = wave - 2; nb * 32 < N; nb += 2) {
#pragma unroll
          for (int e = 0; e < 16; ++e) d[e] = 0.f;
          const float *Pa = P + lk * ldp + nb * 32 + l31, *Ub = U + lk * kLd + l31;
#pragma unroll 8
          for (int r = 0; r < kRows; r += 2) d = __builtin_amdgcn_mfma_f32_32x32x2f32(Pa[r * ldp], Ub[r * kLd], d, 0, 0, 0);
          if (c < C) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
              const int n = nb * 32 + tile_row(e, lane);
              add_through(a.Y + (size_t)sj[n] * C + c, lr * (-d[e] - reg * V[n * kLd + l31]));
            }
          }
        }
      }
      __syncthreads();  // the slice has been consumed
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");  // this thread's adds have been performed
    __syncthreads();
  }

  block_add_counts(correct, masked, a.stats);
}

}  // namespace
}  // namespace imp

using namespace imp;

extern "C" int imp_softmax_update(const imp_intvector *userids, const imp_intvector *itemids, const imp_intvector *indptr,
                                  imp_matrix *X, imp_matrix *Y, float learning_rate, float regularization, int64_t seed,
                                  int negatives, int64_t samples, int64_t *correct, int64_t *masked) {
  return guarded([&] {
    const std::string w("softmax_update");
    if (!userids || !itemids || !indptr || !X || !Y || !correct || !masked) throw std::invalid_argument(w + ": NULL argument");
    if (negatives < 32 || negatives > 256 || negatives % 32) throw std::invalid_argument(w + ": negatives must be a multiple of 32 in 32 .. 256");
    if (X->cols != Y->cols) throw std::invalid_argument("X and Y should have the same number of columns");
    if (X->cols < 2 || X->cols > 1024)
      throw std::invalid_argument(w + ": factor matrices need 2 .. 1024 columns (factors + 1 for the item bias)");
    if (X->itemsize != 4 || Y->itemsize != 4) throw std::invalid_argument(w + ": factor matrices must be float32");
    if (Y->rows > (size_t)INT32_MAX) throw std::invalid_argument(w + ": more than 2^31 - 1 items");
    if (userids->size != itemids->size) throw std::invalid_argument("userids and itemids should have same number of elements");
    if (indptr->size != X->rows + 1) throw std::invalid_argument(w + ": indptr must have X.rows + 1 entries");
    const int64_t nnz = (int64_t)userids->size;
    if (nnz > INT32_MAX) throw std::invalid_argument(w + ": more than 2^31 - 1 nonzeros");
    const int64_t n = samples < 0 ? nnz : samples;
    *correct = *masked = 0;
    if (nnz == 0 || n == 0) return;

    unsigned long long *stats = ctx().pair_stats.reserve(3);
    IMP_CHECK_HIP(hipMemsetAsync(stats, 0, 3 * sizeof(unsigned long long), stream()));
    check_pair_ids("softmax_update", "softmax_check_ids", userids, itemids, indptr, X->rows, Y->rows, stats + 2);
    {
      IMP_PROF("softmax_update");
      // the family's cap on samples in flight (sgd_group.h), in batches of 64; never more workgroups than batches
      const int64_t in_flight = std::max<int64_t>(1, hogwild_in_flight(n, X->rows, Y->rows) / kRows);
      const int grid = (int)std::min<int64_t>({in_flight, (n + kRows - 1) / kRows, (int64_t)ctx().num_cus * 2});
      const size_t lds = softmax_lds_bytes(negatives);
      const SoftmaxArgs a{userids->v.data(), itemids->v.data(), indptr->v.data(), X->mut<float>(), Y->mut<float>(), nnz, n,
                          (uint64_t)seed, learning_rate, regularization, (int)X->cols, (int)Y->rows, negatives, stats};
      auto launch = [&](auto kernel) {
        allow_dynamic_lds(kernel, lds);
        kernel<<<grid, 256, lds, stream()>>>(a);
      };
      switch ((negatives / 16 + 3) / 4) {  // logit tiles per wavefront: 2 N / 32 tiles over 4 wavefronts
        case 1: launch(softmax_update_kernel<1>); break;
        case 2: launch(softmax_update_kernel<2>); break;
        case 3: launch(softmax_update_kernel<3>); break;
        default: launch(softmax_update_kernel<4>); break;
      }
      IMP_CHECK_HIP(hipGetLastError());
    }
    unsigned long long h[2];
    IMP_CHECK_HIP(hipMemcpyAsync(h, stats, sizeof(h), hipMemcpyDeviceToHost, stream()));
    sync();  // synchronous in deferred mode too: the counts are the result
    *correct = (int64_t)h[0];
    *masked = (int64_t)h[1];
  });
}
