// Host-only planner behind csr_schedule.h: validation, the length-sorted row order and the three long-row plans.
#include "csr_schedule.h"

#include <algorithm>
#include <stdexcept>
#include <string>
#include <type_traits>

namespace imp {

template <typename Offset>
void validate_csr(int32_t rows, int32_t cols, int64_t nnz, const Offset *indptr, const int32_t *indices) {
  if (rows < 0 || cols < 0 || nnz < 0) throw std::invalid_argument("negative dimension for CSRMatrix");
  if (std::is_same<Offset, int32_t>::value && nnz > INT32_MAX)
    throw std::invalid_argument("CSRMatrix with more than 2^31-1 nonzeros is not supported");
  if (rows && indptr[rows] != nnz) throw std::invalid_argument("indptr[rows] != nonzeros for CSRMatrix");
  if (rows && indptr[0] != 0) throw std::invalid_argument("indptr[0] != 0 for CSRMatrix");
  // a malformed matrix would turn into out-of-bounds gathers on the device: indptr must not decrease, column ids
  // must lie in [0, cols) (scipy's check_format(full_check=True) conditions; one pass over the host arrays)
  for (int32_t r = 0; r < rows; ++r)
    if (indptr[r + 1] < indptr[r]) throw std::invalid_argument("indptr must be non-decreasing for CSRMatrix (row " + std::to_string(r) + ")");
  int32_t lo = 0, hi = -1;
  for (int64_t k = 0; k < nnz; ++k) {
    lo = std::min(lo, indices[k]);
    hi = std::max(hi, indices[k]);
  }
  if (nnz && (lo < 0 || hi >= cols))
    throw std::invalid_argument("column index out of range for CSRMatrix (" + std::to_string(lo < 0 ? lo : hi) + " not in [0, " +
                                std::to_string(cols) + "))");
}
template void validate_csr<int32_t>(int32_t, int32_t, int64_t, const int32_t *, const int32_t *);
template void validate_csr<int64_t>(int32_t, int32_t, int64_t, const int64_t *, const int32_t *);

std::vector<int32_t> sort_rows_by_length(int32_t rows, const int32_t *indptr, int32_t bin_start[CsrClasses::kBins + 1]) {
  int32_t max_len = 0;
  for (int32_t r = 0; r < rows; ++r) max_len = std::max(max_len, indptr[r + 1] - indptr[r]);
  std::vector<int32_t> count((size_t)max_len + 2, 0);
  for (int32_t r = 0; r < rows; ++r) count[indptr[r + 1] - indptr[r]]++;
  std::vector<int32_t> start((size_t)max_len + 2, 0);
  int32_t acc = 0;
  int32_t class_count[CsrClasses::kBins] = {0};
  for (int32_t len = max_len; len >= 0; --len) {
    start[len] = acc;
    acc += count[len];
    int b = 0;
    while (len <= CsrClasses::kClassMax[b + 1]) ++b;  // kClassMax[b+1] < len <= kClassMax[b]
    class_count[b] += count[len];
  }
  std::vector<int32_t> order((size_t)rows);
  for (int32_t r = 0; r < rows; ++r) order[start[indptr[r + 1] - indptr[r]]++] = r;
  bin_start[0] = 0;
  for (int b = 0; b < CsrClasses::kBins; ++b) bin_start[b + 1] = bin_start[b] + class_count[b];
  return order;
}

// long rows -> segments.
//
// Plain plan: consecutive runs of <= `segment` nonzeros.  Striped plan: the long rows of a popular-item side gather
// the SAME factor rows over and over (C3 item side: 3.3 M long-row nonzeros over 359 K columns), but a plain
// segment spans far more of the factor matrix than an L2 holds, so every pass streams them from the
// Infinity Cache / HBM again.  If the rows are column-sorted and the re-use is >= 4, rows are cut at multiples of
// `stripe` columns instead; the stripes are dealt to the 8 XCDs (greedy by weight) and each XCD's workgroups
// (blockIdx % 8) sweep their stripes one after the other, so that the 2 MB of factor rows a stripe covers are
// fetched into that XCD's L2 and hit by every long row (measured: partial kernel 2.6x faster with fully
// L2-resident gathers; 1.3x with the real plan, whose segments are short).  Segments stay in row-major order (the
// combine kernel sums a row's partials in that fixed order); `seg_exec` is the execution order.
HostPlan build_plan(int32_t cols, const int32_t *indptr, const int32_t *indices, const int32_t *order, int32_t n_plan, int32_t segment,
                    int32_t stripe) {
  if (segment < 1) throw std::invalid_argument("segment length of a long-row plan must be positive");
  const double stripe_reuse = 4.0;  // minimum gathers per column of the gathered matrix for the striped plan
  int64_t long_nnz = 0;
  bool sorted = true;
  for (int32_t li = 0; li < n_plan; ++li) {
    const int32_t r = order[li];
    long_nnz += indptr[r + 1] - indptr[r];
    if (stripe > 0 && sorted) sorted = std::is_sorted(indices + indptr[r], indices + indptr[r + 1]);
  }
  // ... and only when a row still leaves >= 32 nonzeros per stripe on average: with many more stripes than that (configs[3]'s
  // item side: 10 M columns = 814 stripes under rows of ~800 nonzeros) the cut would produce one- and two-entry segments,
  // hundreds of millions of them (23 s of plan building before this rule)
  const int64_t n_stripes_all = stripe > 0 ? ((int64_t)cols + stripe - 1) / stripe : 1;
  HostPlan p;
  p.striped = stripe > 0 && sorted && n_plan > 0 && (double)long_nnz >= stripe_reuse * (double)cols &&
              (double)long_nnz >= 32.0 * (double)n_stripes_all * (double)n_plan;
  p.row_seg.assign((size_t)n_plan + 1, 0);
  std::vector<int32_t> seg_stripe;
  for (int32_t li = 0; li < n_plan; ++li) {
    const int32_t r = order[li];
    p.row_seg[li] = (int32_t)p.seg_row.size();
    int32_t pos = indptr[r];
    const int32_t row_end = indptr[r + 1];
    while (pos < row_end) {
      int32_t hi = row_end, st = 0;
      if (p.striped) {
        st = indices[pos] / stripe;
        const int64_t bound = ((int64_t)st + 1) * stripe;
        hi = (int32_t)(std::lower_bound(indices + pos, indices + row_end, bound, [](int32_t c, int64_t b) { return (int64_t)c < b; }) -
                       indices);
      }
      for (int32_t b = pos; b < hi; b += segment) {
        p.seg_row.push_back(li);
        p.seg_begin.push_back(b);
        p.seg_end.push_back(std::min(hi, b + segment));
        seg_stripe.push_back(st);
      }
      pos = hi;
    }
  }
  const int32_t n_seg = (int32_t)p.seg_row.size();
  p.row_seg[n_plan] = n_seg;
  p.n_long = n_plan;
  p.n_seg = n_seg;
  p.seg_exec.resize((size_t)n_seg);
  if (p.striped) {
    const int32_t n_stripes = (cols + stripe - 1) / stripe;
    std::vector<int64_t> weight((size_t)n_stripes, 0);
    for (int32_t s = 0; s < n_seg; ++s) weight[seg_stripe[s]] += p.seg_end[s] - p.seg_begin[s] + 16;  // + per-segment overhead
    std::vector<int32_t> by_weight((size_t)n_stripes);
    for (int32_t i = 0; i < n_stripes; ++i) by_weight[i] = i;
    std::stable_sort(by_weight.begin(), by_weight.end(), [&](int32_t a, int32_t b) { return weight[a] > weight[b]; });
    int64_t load[8] = {0};
    std::vector<int32_t> stripe_xcd((size_t)n_stripes, 0), stripe_rank((size_t)n_stripes, 0);
    int32_t per_xcd[8] = {0};
    for (int32_t st : by_weight) {  // heaviest first onto the least loaded XCD
      int x = (int)(std::min_element(load, load + 8) - load);
      load[x] += weight[st];
      stripe_xcd[st] = x;
      stripe_rank[st] = per_xcd[x]++;
    }
    for (int32_t s = 0; s < n_seg; ++s) p.seg_exec[s] = s;
    std::stable_sort(p.seg_exec.begin(), p.seg_exec.end(), [&](int32_t a, int32_t b) {
      const int32_t sa = seg_stripe[a], sb = seg_stripe[b];
      if (stripe_xcd[sa] != stripe_xcd[sb]) return stripe_xcd[sa] < stripe_xcd[sb];
      return stripe_rank[sa] < stripe_rank[sb];  // equal stripe: ascending segment id = ascending row
    });
    int32_t posx = 0;
    for (int x = 0; x < 8; ++x) {
      p.xcd_start[x] = posx;
      while (posx < n_seg && stripe_xcd[seg_stripe[p.seg_exec[posx]]] == x) ++posx;
    }
  } else {
    // plain plan: runs of 4 consecutive segments dealt round-robin to the XCDs (neighbouring segments of a row,
    // i.e. neighbouring column ranges, stay on one XCD)
    int32_t posx = 0;
    for (int x = 0; x < 8; ++x) {
      p.xcd_start[x] = posx;
      for (int32_t s = 0; s < n_seg; ++s)
        if ((s / 4) % 8 == x) p.seg_exec[posx++] = s;
    }
  }
  p.xcd_start[8] = n_seg;
  return p;
}

int32_t choose_nm_segment(int64_t long_nnz, const PlanKnobs &knobs) {
  if (knobs.nm_segment > 0) return knobs.nm_segment;
  int32_t seg = 2048;
  while (seg < 16384 && (int64_t)seg * knobs.num_cus * 8 < long_nnz) seg *= 2;
  return seg;
}

HostSchedule plan_csr(int32_t rows, int32_t cols, const int32_t *indptr, const int32_t *indices, const PlanKnobs &knobs) {
  HostSchedule s;
  s.order = sort_rows_by_length(rows, indptr, s.bin_start);
  const int32_t *order = s.order.data();
  auto len = [&](int32_t li) { return indptr[order[li] + 1] - indptr[order[li]]; };
  const int32_t n_long = s.bin_start[1];
  // width: 12288 columns (6 MB of factor rows at f = 128) was the best of {2048 .. 32768} on C3 (359 K columns; narrower
  // = more, shorter segments), 6144 the best of {2048 .. 12288} on the ml-20m shape (138 K columns: the 8 XCDs need
  // enough stripes to balance) -- hence about 24 stripes, between 4096 and 12288 columns
  const int32_t stripe = knobs.stripe >= 0 ? knobs.stripe : std::min(12288, std::max(4096, (cols / 24 + 1023) / 1024 * 1024));
  s.plan_all = build_plan(cols, indptr, indices, order, n_long, knobs.segment, stripe);
  // rows of more than kCholLongRow nonzeros: the first n_chol_long entries of `order` (sorted by descending length)
  while (s.n_chol_long < n_long && len(s.n_chol_long) > CsrClasses::kCholLongRow) ++s.n_chol_long;
  s.plan_chol = build_plan(cols, indptr, indices, order, s.n_chol_long, CsrClasses::kCholSegment, 0);  // never striped
  int64_t long_nnz = 0;
  for (int32_t li = 0; li < n_long; ++li) long_nnz += len(li);
  s.nm_segment = choose_nm_segment(long_nnz, knobs);
  for (int32_t li = 0; li < n_long && len(li) > s.nm_segment; ++li) {  // descending lengths
    s.nm_multi_rows++;
    s.nm_multi_segs += (len(li) + s.nm_segment - 1) / s.nm_segment;
  }
  s.plan_nm = build_plan(cols, indptr, indices, order, n_long, s.nm_segment, 0);  // never striped: a row's segments are consecutive runs
  return s;
}

}  // namespace imp
