// K1q: dispatch of the CG half sweep for f = 64 / 128 over the row-length classes of the schedule (imp_csr::bin_start).
//
// Arithmetic contract: the oracle's CG (implicit/cpu/_als.pyx:152-248).  Kernels -- all on quarter-layout register tiles
// (als_qtile.h), the whole row resident for all 1 + cg_steps passes:
//   short rows (<= 32 nnz)   f = 128: one wavefront per row, 16 rows per workgroup in lock step, the gramian product on the bf16
//                            matrix cores (als_cg_qf.hip als_cg_qfgroup_kernel);  f = 64: independent wavefronts (team width 1,
//                            als_cg_qfteam_kernel, both storages)
//   mid rows (33 .. 512)     a team of wavefronts per row, leader protocol (team_rows, als_qf_common.h): fp32 storage on
//                            32-entry fp32 tiles, 2 / 4 / 8 / 16 wavefronts (als_cg_qf.hip als_cg_qfteam_kernel); float16
//                            storage on 64-entry tiles of packed halves, half the wavefronts (als_cg_qh.hip als_cg_q64team_kernel)
// (The first generation of these kernels -- every wavefront of a team repeating the CG arithmetic, rounds 1-2 -- and the
// IMP_TEAM_FUSED / IMP_SHORT_TEAM1 / IMP_TILE64 switches that selected them were removed in round 6.)
#include <type_traits>

#include "als_qtile.h"
#include "common.h"
#include "long_tail_route.h"

namespace imp {

// als_cg_qf.hip (float16 storage: only the f = 64 short rows go to launch_team_fused)
template <typename T>
void launch_team_fused(const imp_csr *C, int f, int width, int first, int count, T *X, const T *Y, const float *A0, int cg_steps,
                       const char *name);
template <typename T>
void launch_group_fused(const imp_csr *C, int f, int first, int count, T *X, const T *Y, const float *A0, int cg_steps, const char *name);
// als_cg_qh.hip: 64-entry tiles of packed halves, half the wavefronts per row (float16 storage)
template <typename ST>
void launch_team_tile64(const imp_csr *C, int f, int width, int first, int count, ST *X, const ST *Y, const float *A0, int cg_steps,
                        const char *name);

// als_cg_qf.hip: the classes of team widths 8, 4 and 2 in one persistent launch, rows drawn by ticket (fp32 storage); `finish`
// (or null): the long rows of more than one segment, finished at the head of the launch
template <typename T>
void launch_team_chain(const imp_csr *C, int f, const int (&first)[3], const int (&count)[3], T *X, const T *Y, const float *A0, int cg_steps,
                       const char *name, const NmTail *finish);
// als_cg_qf.hip: (256,512] and the short rows -- the two 1024-thread classes -- in one persistent launch (fp32 storage, f = 128);
// `fixup` (or null): the fix list of the long rows, re-solved at the head of the launch
template <typename T>
void launch_wide_chain(const imp_csr *C, int f, const int (&first)[2], const int (&count)[2], T *X, const T *Y, const float *A0, int cg_steps,
                       const char *name, const NmTail *fixup);

template <int F, typename T> static void run_classes_q(const imp_csr *C, T *X, const T *Y, const float *A0, int cg_steps, const NmTail &tail) {
  const int32_t *b = C->bin_start;  // classes: 1 (256,512]  2 (128,256]  3 (64,128]  4 (32,64]  5 (16,32]  6 (0,16]
  constexpr bool kHalf = std::is_same<T, __half>::value;
  // the stand-alone fix-up of the rows the long-row path listed (normally none: the kernel reads a zero and exits)
  auto fixup_alone = [&]() {
    launch_cg_fixup<F, T>(reinterpret_cast<const unsigned *>(tail.ctl + 2), tail.fix_rows, tail.capacity, C, X, Y, A0, cg_steps);
  };
  // team width per class: a wavefront holds 32 entries (fp32 storage) or 64 (packed halves)
  auto team = [&](int width32, int lo, int hi, const char *name) {
    if constexpr (kHalf) launch_team_tile64<T>(C, F, width32 / 2, lo, hi - lo, X, Y, A0, cg_steps, name);
    else launch_team_fused<T>(C, F, width32, lo, hi - lo, X, Y, A0, cg_steps, name);
  };
  // fp32 storage at f = 128 chains (128,256], (64,128], (32,64] in one launch and (256,512] with the short rows in another.  A
  // profiled run with no name filter -- a per-kernel pass, which wants a scope per class -- keeps the per-class launches, as do
  // float16 storage (packed tiles) and f = 64 (launch_team_chain has the reason).
  const bool chained = F == 128 && !kHalf && !prof_unfiltered();
  const int first[3] = {b[2], b[3], b[4]}, count[3] = {b[3] - b[2], b[4] - b[3], b[5] - b[4]};
  const int wide_first[2] = {b[1], b[5]}, wide_count[2] = {b[2] - b[1], b[7] - b[5]};
  // The tail of the long-row path (long_tail_route.h): on the chained route its two parts ride the chains' heads; everywhere
  // else, and where a chain has no rows of its own, they are the stand-alone launches in their old order.
  const LongTailRoute route = long_tail_route(count, wide_count, tail.n_multi, tail.capacity, chained);
  if (route.finish == LongTailRoute::kFinishAlone) cg_nm_finish<T>(tail, X, F, cg_steps);
  if (route.fixup == LongTailRoute::kFixupAheadOfClasses) fixup_alone();
  if (chained) {
    launch_team_chain<T>(C, F, first, count, X, Y, A0, cg_steps, "als_cg_team_chain_rows",
                         route.finish == LongTailRoute::kFinishInTeamChain ? &tail : nullptr);
    if (route.fixup == LongTailRoute::kFixupBehindTeamChain) fixup_alone();
    launch_wide_chain<T>(C, F, wide_first, wide_count, X, Y, A0, cg_steps, "als_cg_wide_chain_rows",
                         route.fixup == LongTailRoute::kFixupInWideChain ? &tail : nullptr);
    return;
  }
  team(16, b[1], b[2], "als_cg_team16_rows");  // (names: the row class)
  team(8, b[2], b[3], "als_cg_team8_rows");
  team(4, b[3], b[4], "als_cg_team4_rows");
  team(2, b[4], b[5], "als_cg_team2_rows");
  // short rows.  f = 128: 16 rows per workgroup in lock step with the gramian product on the matrix cores (measured 1.16 ms per
  // configs[2] iteration against 1.38 ms for independent waves with the VALU product -- at f = 128 the product is 57 % of a short
  // row's arithmetic); f = 64: independent waves win (configs[1] shape: 0.84 against 0.94 ms), the product is a quarter of the size
  if constexpr (F == 64) launch_team_fused<T>(C, F, 1, b[5], b[7] - b[5], X, Y, A0, cg_steps, "als_cg_short_rows");
  else launch_group_fused<T>(C, F, b[5], b[7] - b[5], X, Y, A0, cg_steps, "als_cg_short_rows");
}

template <typename T> void least_squares_cg_q(const imp_csr *C, T *X, const T *Y, const float *A0, int f, int cg_steps, const NmTail &tail) {
  if (f == 128) run_classes_q<128, T>(C, X, Y, A0, cg_steps, tail);
  else if (f == 64) run_classes_q<64, T>(C, X, Y, A0, cg_steps, tail);
  else throw std::invalid_argument("least_squares_cg_q: f must be 64 or 128");
}
template void least_squares_cg_q<float>(const imp_csr *, float *, const float *, const float *, int, int, const NmTail &);
template void least_squares_cg_q<__half>(const imp_csr *, __half *, const __half *, const float *, int, int, const NmTail &);

}  // namespace imp
