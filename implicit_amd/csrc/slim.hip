// K20: the fit of SLIM: imp_slim_solve, `items` independent elastic-net problems in Gram form by cyclic coordinate
// descent, defined operation for operation in include/implicit_hip.h.  No floating-point atomics: equal inputs give equal bits.
//
// slim_diag_kernel       the diagonal of A is checked (the smallest failing item goes to the fail word) and copied aside.
// slim_cd_kernel         one workgroup of kSlimBlock threads per column j, columns drawn from a ticket counter in descending order
//   of A[j][j] (the popular items have the largest supports and the most sweeps; no workgroup waits for another).  r (items floats)
//   lives in the dynamic LDS; w is the column's own output row W[j][.], which is contiguous, and thread t is the only one that
//   ever touches the entries i = t (mod kSlimBlock) of it.  A sweep walks the coordinates in chunks of kSlimBlock: every thread
//   evaluates its coordinate against the current r; the lowest coordinate of the chunk with d != 0 is found with one ballot per
//   wavefront and one word per wavefront in the LDS; every thread adds d A[i][.] into r; the coordinates after it are evaluated
//   again.  A coordinate with d = 0 changes nothing, so this is the sequential rule bit for bit, and a chunk without an active
//   coordinate costs one evaluation and one barrier.
// slim_transpose_kernel  in-place tiled transpose of the square matrix: W[j][i] (column j's w) becomes W[i][j], the layout of B.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <numeric>

#include "common.h"

namespace imp {

namespace {
constexpr int kSlimBlock = 1024, kSlimWaves = kSlimBlock / 64;
// after r in the dynamic LDS: [2][kSlimWaves] candidate positions, [2][kSlimWaves] their d, [kSlimWaves] maxima, the ticket drawn
constexpr int kSlimScratchWords = 5 * kSlimWaves + 4;
constexpr int kSlimStatWords = 8;  // after order and sweeps in the workspace: the ticket, pad, updates (64 bit), longest column (64 bit)
constexpr int kNoCandidate = INT_MAX;

size_t slim_lds_bytes(size_t n) { return ((n + 3) / 4 * 4 + kSlimScratchWords) * sizeof(float); }
static_assert(((size_t)IMP_SLIM_MAX_ITEMS + kSlimScratchWords) * sizeof(float) <= 160 * 1024, "r and the scratch share one workgroup's LDS");

__global__ void slim_diag_kernel(const float *__restrict__ A, long n, float *__restrict__ diag, unsigned long long *__restrict__ failed) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const float d = A[j * n + j];
  diag[j] = d;
  if (!(d > 0.f) || !isfinite(d)) atomicMin(failed, (unsigned long long)j);
}

__global__ __launch_bounds__(kSlimBlock) void slim_cd_kernel(const float *__restrict__ A, const float *__restrict__ diag,
                                                             const int32_t *__restrict__ order, int n, int n_pad, float l1, int positive,
                                                             int max_sweeps, float tol, float *__restrict__ W, int32_t *__restrict__ sweeps,
                                                             int *__restrict__ ticket, unsigned long long *__restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) float slim_lds[];
  float *r = slim_lds;                                 // [n]
  int *s_cand = reinterpret_cast<int *>(r + n_pad);    // [2][kSlimWaves]
  float *s_d = r + n_pad + 2 * kSlimWaves;             // [2][kSlimWaves]
  float *s_max = r + n_pad + 4 * kSlimWaves;           // [kSlimWaves]
  int *s_col = reinterpret_cast<int *>(r + n_pad + 5 * kSlimWaves);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned step = 0;  // evaluations so far: its low bit selects the half of s_cand / s_d, so that a workgroup that has read "no
                      // candidate" and moved on never writes the half a slower wavefront is still reading
  for (;;) {
    if (tid == 0) *s_col = atomicAdd(ticket, 1);
    __syncthreads();
    const int slot = *s_col;
    if (slot >= n) break;
    const int j = order[slot];
    const float *Aj = A + (size_t)j * n;
    float *w = W + (size_t)j * n;
    for (int k = tid; k < n; k += kSlimBlock) r[k] = 0.f, w[k] = 0.f;
    __syncthreads();  // r is zero; and every thread has read s_col before the next ticket is written
    const long long t0 = tid == 0 ? wall_clock64() : 0;
    unsigned long long updates = 0;
    int s = 1;
    for (;; ++s) {
      float dmax = 0.f, wmax = 0.f;
      for (int c0 = 0; c0 < n; c0 += kSlimBlock) {
        const int i = c0 + tid;
        const bool live = i < n && i != j;
        float a = 1.f, aji = 0.f, wi = 0.f;
        if (live) a = diag[i], aji = Aj[i], wi = w[i];
        int lo = 0;  // positions below it are final for this sweep
        for (;;) {
          float nw = wi, d = 0.f;
          if (live && tid >= lo) {
            const float rho = (aji - r[i]) + a * wi;
            if (positive) {
              const float t = rho - l1;
              nw = t > 0.f ? t / a : 0.f;
            } else {
              nw = rho > l1 ? (rho - l1) / a : rho < -l1 ? (rho + l1) / a : 0.f;
            }
            d = nw - wi;
          }
          const unsigned long long moved = __ballot(d != 0.f);
          const int half = (int)(step++ & 1u) * kSlimWaves;
          if (moved) {
            if (lane == __ffsll((long long)moved) - 1) s_cand[half + wave] = tid, s_d[half + wave] = d;
          } else if (lane == 0) {
            s_cand[half + wave] = kNoCandidate;
          }
          __syncthreads();
          int first = kNoCandidate;
          float df = 0.f;
          for (int q = 0; q < kSlimWaves; ++q) {
            const int c = s_cand[half + q];
            if (c != kNoCandidate) {
              first = c, df = s_d[half + q];
              break;
            }
          }
          if (first == kNoCandidate) break;
          if (tid == first) wi = nw, w[i] = nw;
          const float *Ai = A + (size_t)(c0 + first) * n;
#pragma unroll 4  // four loads of the row in flight per thread
          for (int k = tid; k < n; k += kSlimBlock) r[k] = r[k] + df * Ai[k];
          dmax = fmaxf(dmax, fabsf(df));
          ++updates;
          lo = first + 1;
          __syncthreads();  // r is updated before anybody evaluates against it
        }
        wmax = fmaxf(wmax, fabsf(wi));
      }
      for (int o = 32; o > 0; o >>= 1) wmax = fmaxf(wmax, __shfl_xor(wmax, o));
      if (lane == 0) s_max[wave] = wmax;
      __syncthreads();  // the next write of s_max is behind the barrier of at least one more evaluation
      for (int q = 0; q < kSlimWaves; ++q) wmax = fmaxf(wmax, s_max[q]);
      if (dmax <= tol * wmax || s == max_sweeps) break;
    }
    if (tid == 0) {
      sweeps[j] = s;
      atomicAdd(&stats[0], updates);
      atomicMax(&stats[1], (unsigned long long)(wall_clock64() - t0));
    }
  }
}

constexpr int kTile = 32;
// grid (tiles, tiles), 256 threads; the workgroup of tile (bi, bj), bi <= bj, swaps it with tile (bj, bi)
__global__ __launch_bounds__(256) void slim_transpose_kernel(float *__restrict__ W, int n) {
  __shared__ float ta[kTile][kTile + 1], tb[kTile][kTile + 1];
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj < bi) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int r0 = bi * kTile, c0 = bj * kTile;
  for (int y = ty; y < kTile; y += 8) {
    if (r0 + y < n && c0 + tx < n) ta[y][tx] = W[(size_t)(r0 + y) * n + c0 + tx];
    if (bi != bj && c0 + y < n && r0 + tx < n) tb[y][tx] = W[(size_t)(c0 + y) * n + r0 + tx];
  }
  __syncthreads();
  for (int y = ty; y < kTile; y += 8) {
    if (c0 + y < n && r0 + tx < n) W[(size_t)(c0 + y) * n + r0 + tx] = ta[tx][y];
    if (bi != bj && r0 + y < n && c0 + tx < n) W[(size_t)(r0 + y) * n + c0 + tx] = tb[tx][y];
  }
}
}  // namespace

}  // namespace imp

using namespace imp;

extern "C" int imp_slim_solve(const imp_matrix *A, float l1, int positive, int max_sweeps, float tol, imp_matrix *W, int32_t *sweeps) {
  return guarded([&] {
    if (!A || !W) throw std::invalid_argument("slim_solve: NULL argument");
    if (A->itemsize != 4 || W->itemsize != 4 || A->rows != A->cols || W->rows != W->cols || A->rows != W->rows)
      throw std::invalid_argument("slim_solve: A and W must be square float32 matrices of the same order");
    if (A->overlaps(W)) throw std::invalid_argument("slim_solve: A and W must not share storage");
    if (!std::isfinite(l1) || l1 < 0.f) throw std::invalid_argument("slim_solve: l1 must be finite and >= 0");
    if (!std::isfinite(tol) || tol < 0.f) throw std::invalid_argument("slim_solve: tol must be finite and >= 0");
    if (max_sweeps < 1) throw std::invalid_argument("slim_solve: max_sweeps must be >= 1");
    const size_t n = A->rows;
    if (n == 0) return;
    if (n > (size_t)IMP_SLIM_MAX_ITEMS)
      throw std::invalid_argument("slim_solve: " + std::to_string(n) + " items, at most " + std::to_string(IMP_SLIM_MAX_ITEMS) +
                                  " are supported (a column's running product has to fit one workgroup's LDS)");
    auto &c = ctx();
    float *diag = c.slim_diag.reserve(n);
    int32_t *order = c.slim_ws.reserve(2 * n + kSlimStatWords);
    int32_t *d_sweeps = order + n;
    int *words = reinterpret_cast<int *>(order + 2 * n);  // an even word offset: the two 64-bit counts behind the ticket are 8-byte aligned
    unsigned long long *stats = reinterpret_cast<unsigned long long *>(words + 2);
    std::vector<float> h_diag(n);
    std::vector<int32_t> h_order(n);
    {
      IMP_PROF("slim_diag");
      unsigned long long *failed = reset_fail_word();
      slim_diag_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream()>>>(A->f32(), (long)n, diag, failed);
      IMP_CHECK_HIP(hipGetLastError());
      IMP_CHECK_HIP(hipMemcpyAsync(h_diag.data(), diag, n * sizeof(float), hipMemcpyDeviceToHost, stream()));
      const int64_t bad = read_fail_word(failed);
      if (bad >= 0)
        throw std::invalid_argument("slim_solve: the diagonal entry of item " + std::to_string(bad) + " is not finite or not > 0");
    }
    std::iota(h_order.begin(), h_order.end(), 0);
#ifndef IMP_SLIM_NO_ORDER  // timing-only build variant (profiles/slim_bench.py): the columns in index order
    std::stable_sort(h_order.begin(), h_order.end(), [&](int32_t x, int32_t y) { return h_diag[x] > h_diag[y]; });
#endif
    IMP_CHECK_HIP(hipMemcpyAsync(order, h_order.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, stream()));
    sync();  // no copy from or to the two host vectors is queued past this line: a failure below may unwind them
    IMP_CHECK_HIP(hipMemsetAsync(words, 0, 6 * sizeof(int), stream()));
    float *const w = W->mut<float>();
    const size_t lds = slim_lds_bytes(n);
    allow_dynamic_lds(slim_cd_kernel, lds);
    {
      IMP_PROF("slim_cd");
      const unsigned grid = (unsigned)std::min(n, (size_t)2 * c.num_cus);
      slim_cd_kernel<<<grid, kSlimBlock, lds, stream()>>>(A->f32(), diag, order, (int)n, (int)((n + 3) / 4 * 4), l1, positive ? 1 : 0,
                                                          max_sweeps, tol, w, d_sweeps, words, stats);
      IMP_CHECK_HIP(hipGetLastError());
    }
    {
      IMP_PROF("slim_transpose");
      const unsigned tiles = (unsigned)((n + kTile - 1) / kTile);
      slim_transpose_kernel<<<dim3(tiles, tiles), 256, 0, stream()>>>(w, (int)n);
      IMP_CHECK_HIP(hipGetLastError());
    }
    if (sweeps) IMP_CHECK_HIP(hipMemcpyAsync(sweeps, d_sweeps, n * sizeof(int32_t), hipMemcpyDeviceToHost, stream()));
    sync();
    c.slim_items = n;
  });
}

extern "C" int imp_slim_stats(unsigned long long *updates, double *longest_column_seconds) {
  return guarded([&] {
    auto &c = ctx();
    sync();
    unsigned long long h[2] = {0, 0};
    if (c.slim_items && c.slim_ws.size >= 2 * c.slim_items + kSlimStatWords) {
      const size_t n = c.slim_items;
      IMP_CHECK_HIP(hipMemcpyAsync(h, c.slim_ws.data() + 2 * n + 2, sizeof(h), hipMemcpyDeviceToHost, stream()));
      sync();
    }
    int rate_khz = 100000;  // wall_clock64 ticks per millisecond
    IMP_CHECK_HIP(hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, c.device));
    if (updates) *updates = h[0];
    if (longest_column_seconds) *longest_column_seconds = (double)h[1] / ((double)rate_khz * 1e3);
  });
}
