// Dense symmetric helpers shared by spd_inverse.hip and ease.hip (internal, not part of the C-ABI).
#ifndef IMPLICIT_AMD_CSRC_SPD_INVERSE_H_
#define IMPLICIT_AMD_CSRC_SPD_INVERSE_H_
#include <cstddef>

namespace imp {
// A[r][c] = A[c][r] for every r < c of the n x n fp32 matrix A (one launch on the library stream): the upper triangle becomes a
// bitwise copy of the lower one.
void mirror_lower(float *A, size_t n);
}  // namespace imp
#endif  // IMPLICIT_AMD_CSRC_SPD_INVERSE_H_
