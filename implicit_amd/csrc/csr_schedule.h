// Row schedule and long-row plans of a CSRMatrix: pure host arithmetic over indptr / indices (no device code, no HIP
// header), so that it can be read and tested without a GPU.  imp_csr_create uploads what plan_csr returns;
// imp_host_csr_plan hands the same arrays to the caller.
#ifndef IMPLICIT_AMD_CSRC_CSR_SCHEDULE_H_
#define IMPLICIT_AMD_CSRC_CSR_SCHEDULE_H_

#include <cstdint>
#include <vector>

namespace imp {

// Length classes and segment sizes of the schedule (imp_csr derives from this; the class table is explained there).
struct CsrClasses {
  static constexpr int kBins = 8;
  static constexpr int kShortRow = 32;
  static constexpr int kLongRow = 512;
  static constexpr int kSegment = 512;
  static constexpr int32_t kClassMax[kBins + 1] = {INT32_MAX, 512, 256, 128, 64, 32, 16, 0, -1};
  static constexpr int kCholLongRow = 1024, kCholSegment = 1024;
};

struct PlanKnobs {
  int32_t segment = CsrClasses::kSegment;  // nonzeros per segment of plan_all
  int32_t stripe = -1;                     // column-stripe width of plan_all; < 0: automatic, 0: never striped
  int32_t nm_segment = 0;                  // nonzeros per segment of plan_nm; 0: automatic
  int32_t num_cus = 256;                   // compute units of the device (automatic nm_segment)
};

// The first n_long entries of `order` cut into segments.  Segments are numbered in row-major order (a row's partials are
// summed in that fixed order); `seg_exec` is the order they are executed in.
struct HostPlan {
  int32_t n_long = 0, n_seg = 0;
  std::vector<int32_t> row_seg;    // [n_long + 1] first segment of each long row
  std::vector<int32_t> seg_row;    // [n_seg]      long-row index of each segment
  std::vector<int32_t> seg_begin;  // [n_seg]      nonzero range of each segment
  std::vector<int32_t> seg_end;    // [n_seg]
  std::vector<int32_t> seg_exec;   // [n_seg]      segment ids grouped by XCD
  int32_t xcd_start[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // seg_exec[xcd_start[x] .. xcd_start[x+1]) belongs to XCD x
  bool striped = false;
};

struct HostSchedule {
  std::vector<int32_t> order;  // row ids by descending length, ascending id within a length
  int32_t bin_start[CsrClasses::kBins + 1] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  HostPlan plan_all, plan_chol, plan_nm;  // see imp_csr
  int32_t n_chol_long = 0;
  int32_t nm_segment = 2048, nm_multi_rows = 0, nm_multi_segs = 0;
};

// Throws std::invalid_argument for what would turn into out-of-bounds accesses later.  Offset = int32_t or int64_t.
template <typename Offset>
void validate_csr(int32_t rows, int32_t cols, int64_t nnz, const Offset *indptr, const int32_t *indices);

// Counting sort of the row ids by descending length (stable), and the cut of the sorted rows into the length classes.
std::vector<int32_t> sort_rows_by_length(int32_t rows, const int32_t *indptr, int32_t bin_start[CsrClasses::kBins + 1]);

// order[0 .. n_plan) cut into segments of <= `segment` nonzeros, at multiples of `stripe` columns when stripe > 0 and the
// rows qualify (csr_schedule.hip).
HostPlan build_plan(int32_t cols, const int32_t *indptr, const int32_t *indices, const int32_t *order, int32_t n_plan, int32_t segment,
                    int32_t stripe);

// Segment length of plan_nm for `long_nnz` nonzeros in long rows.
int32_t choose_nm_segment(int64_t long_nnz, const PlanKnobs &knobs);

// The whole schedule of a validated matrix.
HostSchedule plan_csr(int32_t rows, int32_t cols, const int32_t *indptr, const int32_t *indices, const PlanKnobs &knobs);

}  // namespace imp

#endif  // IMPLICIT_AMD_CSRC_CSR_SCHEDULE_H_
