// K8: RandomState -- uniform / normal factor initialisation on the device.
//
// Replaces implicit/gpu/random.cu:14-40 (cuRAND default generator + Thrust affine rescale) with a
// counter-based Philox4x32-10 kernel: element i of draw d is a pure function of (seed, d, i), so the
// result does not depend on the launch geometry.  PARITY UNPINNED by design: neither cuRAND's stream
// nor the CPU path's numpy Generator is reproduced (no reference test depends on specific random
// values); parity runs inject identical initial factors from the host instead.
#include "common.h"
#include "philox.h"

namespace imp {

// (0, 1]: from 2^23 on, k + 0.5f is a tie that rounds to the even neighbour, and 16777215 + 0.5f rounds to 2^24 -- the 256 words
// with their top 24 bits set give exactly 1.0 (uniform() then returns `high`, normal_kernel a zero radius: log(1) = 0, finite)
__device__ __forceinline__ float u01(uint32_t x) { return ((x >> 8) + 0.5f) * (1.0f / 16777216.0f); }

__global__ void uniform_kernel(float *__restrict__ out, size_t n, uint64_t seed, uint32_t draw, float low, float high) {
  size_t quads = (n + 3) / 4;
  for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < quads; q += (size_t)gridDim.x * blockDim.x) {
    u32x4 r = philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), draw, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
    float v[4] = {u01(r.x), u01(r.y), u01(r.z), u01(r.w)};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * q + j < n) out[4 * q + j] = low + (high - low) * v[j];
  }
}

__global__ void normal_kernel(float *__restrict__ out, size_t n, uint64_t seed, uint32_t draw, float mean, float stddev) {
  size_t quads = (n + 3) / 4;
  for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < quads; q += (size_t)gridDim.x * blockDim.x) {
    u32x4 r = philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), draw, 1u, (uint32_t)seed, (uint32_t)(seed >> 32));
    float u[4] = {u01(r.x), u01(r.y), u01(r.z), u01(r.w)};
    float v[4];
    float m0 = sqrtf(-2.f * logf(u[0])), m1 = sqrtf(-2.f * logf(u[2]));
    v[0] = m0 * cosf(6.2831853071795865f * u[1]);
    v[1] = m0 * sinf(6.2831853071795865f * u[1]);
    v[2] = m1 * cosf(6.2831853071795865f * u[3]);
    v[3] = m1 * sinf(6.2831853071795865f * u[3]);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * q + j < n) out[4 * q + j] = mean + stddev * v[j];
  }
}

}  // namespace imp

using namespace imp;

struct imp_random {
  uint64_t seed = 42;
  uint32_t draws = 0;
};

extern "C" {

int imp_random_create(int64_t seed, imp_random **out) {
  return guarded([&] {
    (void)ctx();
    auto r = new imp_random();
    r->seed = (uint64_t)seed;
    *out = r;
  });
}
int imp_random_destroy(imp_random *r) {
  return guarded([&] { delete r; });
}

int imp_random_uniform(imp_random *r, size_t rows, size_t cols, float low, float high, imp_matrix **out) {
  return guarded([&] {
    std::unique_ptr<imp_matrix> m(new_matrix(rows, cols, 4, false));
    size_t n = rows * cols;
    if (n) {
      IMP_PROF("rng_uniform");
      int grid = (int)std::min<size_t>((n / 4 + 255) / 256 + 1, (size_t)ctx().num_cus * 8);
      uniform_kernel<<<grid, 256, 0, stream()>>>(m->mut<float>(), n, r->seed, r->draws++, low, high);
      IMP_CHECK_HIP(hipGetLastError());
    }
    sync();
    *out = m.release();
  });
}

int imp_random_randn(imp_random *r, size_t rows, size_t cols, float mean, float stddev, imp_matrix **out) {
  return guarded([&] {
    std::unique_ptr<imp_matrix> m(new_matrix(rows, cols, 4, false));
    size_t n = rows * cols;
    if (n) {
      IMP_PROF("rng_normal");
      int grid = (int)std::min<size_t>((n / 4 + 255) / 256 + 1, (size_t)ctx().num_cus * 8);
      normal_kernel<<<grid, 256, 0, stream()>>>(m->mut<float>(), n, r->seed, r->draws++, mean, stddev);
      IMP_CHECK_HIP(hipGetLastError());
    }
    sync();
    *out = m.release();
  });
}

}  // extern "C"
