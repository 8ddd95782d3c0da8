// Counter-based Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), shared by the
// device RandomState (random.hip), the BPR and WARP samplers (bpr.hip, warp.hip) and the LMF negatives (lmf.hip).  A draw is a pure function
// of (counter, key), so a kernel's random stream does not depend on its launch geometry.  The fourth counter word tags the user:
//   0  RandomState::uniform    1  RandomState::randn    2  bpr_update sample pairs    3  lmf_update negatives
//   4  warp_update positives and candidates
#ifndef IMPLICIT_AMD_CSRC_PHILOX_H_
#define IMPLICIT_AMD_CSRC_PHILOX_H_
#include <hip/hip_runtime.h>

#include <cstdint>

namespace imp {

struct u32x4 {
  uint32_t x, y, z, w;
};

__device__ __forceinline__ u32x4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
    uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
    c0 = n0, c1 = n1, c2 = n2, c3 = n3;
    k0 += W0, k1 += W1;
  }
  return {c0, c1, c2, c3};
}

}  // namespace imp
#endif  // IMPLICIT_AMD_CSRC_PHILOX_H_
