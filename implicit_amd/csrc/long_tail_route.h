// Who runs the tail of the long-row path of a CG half sweep (als_cg_nm.hip): pure host arithmetic (no device code, no HIP
// header), so that it can be read and tested without a GPU (imp_host_long_tail_route).
//
// Behind als_cg_nm_kernel two pieces of work are pending: the rows of more than one segment have to be FINISHED (their partial
// images summed in segment order, the CG run on the sum), and the rows a normal-matrix solve listed -- operands beyond the fp16
// range -- have to be re-solved in fp32 (the FIX-UP; normally the list is empty).  As launches of their own they are three
// nearly empty kernels and their gaps on the critical path of the half sweep.  Where fp32 storage at f = 128 takes the chained
// launches (als_cg_qf.hip) they ride those instead, each behind a kernel boundary that is there anyway:
//   * the finish items at the head of the chain of the three 512-thread classes, before its gramian is staged;
//   * the fix-up at the head of the chain of the two 1024-thread classes: every launch that can list a row -- the
//     normal-matrix kernel and whoever finishes -- has ended by then.
// A chain that has no rows of its own is not launched, and its passenger falls back to the stand-alone kernels, queued where
// they were before: reduce + finish ahead of the classes, the fix-up behind the last launch that can list a row.
#ifndef IMPLICIT_AMD_CSRC_LONG_TAIL_ROUTE_H_
#define IMPLICIT_AMD_CSRC_LONG_TAIL_ROUTE_H_

#include <cstdint>

namespace imp {

struct LongTailRoute {
  enum Finish : int32_t { kNoFinish = 0, kFinishAlone = 1, kFinishInTeamChain = 2 };
  enum Fixup : int32_t {
    kNoFixup = 0,
    kFixupAheadOfClasses = 1,    // stand-alone, behind the normal-matrix kernel and the stand-alone finish (nothing later lists)
    kFixupBehindTeamChain = 2,   // stand-alone, behind the team chain that carried the finish items
    kFixupInWideChain = 3
  };
  int32_t finish = kNoFinish, fixup = kNoFixup;
};

// chain[3]: rows of (128,256], (64,128], (32,64]; wide[2]: rows of (256,512] and short rows; n_multi: rows of more than one
// segment; capacity: entries of the fix list (the long rows of the plan; 0: no normal-matrix launch); chained: the half sweep
// takes launch_team_chain / launch_wide_chain (run_classes_q)
inline LongTailRoute long_tail_route(const int32_t (&chain)[3], const int32_t (&wide)[2], int32_t n_multi, int32_t capacity, bool chained) {
  const bool team_chain = chained && (chain[0] > 0 || chain[1] > 0 || chain[2] > 0);
  const bool wide_chain = chained && (wide[0] > 0 || wide[1] > 0);
  LongTailRoute r;
  if (n_multi > 0) r.finish = team_chain ? LongTailRoute::kFinishInTeamChain : LongTailRoute::kFinishAlone;
  if (capacity > 0) {
    if (wide_chain) r.fixup = LongTailRoute::kFixupInWideChain;
    else r.fixup = r.finish == LongTailRoute::kFinishInTeamChain ? LongTailRoute::kFixupBehindTeamChain : LongTailRoute::kFixupAheadOfClasses;
  }
  return r;
}

}  // namespace imp

#endif  // IMPLICIT_AMD_CSRC_LONG_TAIL_ROUTE_H_
