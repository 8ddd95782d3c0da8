// The select half of the top-k scorer (topk.hip): every kernel that turns scores or candidate lists into the k best of a
// row, on the primitives of select_ops.h.
//   select_kernel                     a whole score row: radix select, the reference heap's tie rule, sort
//   select_pruned_kernel              a score row with tile maxima (materialising path): only the tiles that can matter
//   subset_threshold*_kernel          the emit path's threshold tau[q] from the pre-pass subset
//   select_candidates_kernel          the emit path's candidate lists
//   select_screened_kernel            the screened emit path's lists: re-scores the few entries that can be among the best k
// The scoring kernels (topk.hip, topk_resident.h) meet them at the tile maxima (kTileItems) and at EmitArgs.
#ifndef IMPLICIT_AMD_CSRC_TOPK_SELECT_H_
#define IMPLICIT_AMD_CSRC_TOPK_SELECT_H_
#include <cfloat>
#include <cstdint>

#include "als_qtile.h"  // load4: fp32 / fp16 factor storage converted in registers
#include "select_ops.h"
#include "wave_ops.h"  // wave_allmax_u32

namespace imp {

constexpr int kTileItems = 64;  // granularity of the tile maxima

// what an emit pass (score_gemm_direct_kernel MODE 2, score_resident_kernel MODE 2 / 3) is given and leaves for the selects
struct EmitArgs {
  const uint32_t *tau;        // [nq] ordered key of the query's threshold
  const uint32_t *row_bits;   // [nq][words] per-query filter bitmap (may be null)
  const uint32_t *item_bits;  // [words] global item filter bitmap (may be null)
  int words;
  uint64_t *cand;             // [nq][cap]
  unsigned int *count;        // [nq]
  int cap;
  float *row_unscale;         // [nq] resident form: the keys carry raw accumulators; factor that turns a row's into scores (else null)
  float *row_eps;             // [nq] screened emit pass (MODE 3): the error bound of the row's one-product accumulators (else null)
};

// ---- the tie rule ----------------------------------------------------------------------------------------------------------
// More entries tie with the k-th score t than there are places left: which of them stay is decided by the order in which the
// reference's heap (implicit/cpu/select.h:12-40) met them.  It walks the row in column order.  Tied entries enter until the
// heap holds k entries >= t; the column at which that happens is the saturation column s = the column of the k-th entry >= t
// in column order.  A tied entry after s never enters.  Each later entry > t then evicts the heap's minimum, which among
// equal scores is the tied entry with the LOWEST column.  So the surviving ties are
//     the tied columns <= s, minus the e lowest of them,   e = #{column > s : score > t},
// and with the entries > t they are exactly k.  Two functions evaluate this closed form, on the two layouts it is needed for:
// select_row_ties reads a score row in column order (ballots and popcounts over 64 columns at a time), write_best_k a
// candidate list sorted by (score desc, column desc) that holds every entry >= t.

// Row form (select_kernel): appends the k winners of a row whose k-th ordered score is t32 -- everything above it and the
// surviving ties -- to cand[0 .. kpad), unsorted.  *sh_count is the append cursor, zero and behind a barrier on entry.
template <int BLOCK>
__device__ __forceinline__ void select_row_ties(const float *__restrict__ row, int ni, int k, int kpad, uint32_t t32, uint64_t *cand,
                                                unsigned int *sh_count) {
  const int tid = threadIdx.x;
  __shared__ int sh_s;
  __shared__ unsigned int sh_e;
  if (tid < 64) {
    unsigned int running = 0, e = 0;
    int s_col = -1;
    for (int c0 = 0; c0 < ni; c0 += 64) {
      const int c = c0 + tid;
      const uint32_t key = c < ni ? ordered(row[c]) : 0u;
      const bool ge = c < ni && key >= t32, gt = c < ni && key > t32;
      const unsigned long long m_ge = __ballot(ge), m_gt = __ballot(gt);
      if (s_col < 0) {
        const unsigned int cnt = __popcll(m_ge);
        if (running + cnt >= (unsigned)k) {
          const unsigned int need = k - running;  // the need-th set bit of m_ge is the saturation column
          const unsigned int incl = __popcll(m_ge & ((2ull << tid) - 1ull));
          const unsigned long long hit = __ballot(ge && incl == need);
          const int L = __ffsll((long long)hit) - 1;
          s_col = c0 + L;
          e += __popcll(m_gt & ~((2ull << L) - 1ull));
        } else {
          running += cnt;
        }
      } else {
        e += __popcll(m_gt);
      }
    }
    if (tid == 0) {
      sh_s = s_col;
      sh_e = e;
    }
  }
  __syncthreads();
  for (int i = tid; i < ni; i += BLOCK) {  // everything strictly above the tie score
    const float sc = row[i];
    if (ordered(sc) > t32) {
      unsigned int slot = atomicAdd(sh_count, 1u);
      if (slot < (unsigned)kpad) cand[slot] = make_key(sc, i);
    }
  }
  if (tid < 64) {  // the surviving ties, ranked by column
    const int s_col = sh_s;
    const unsigned int e = sh_e;
    unsigned int seen = 0;
    for (int c0 = 0; c0 <= s_col; c0 += 64) {
      const int c = c0 + tid;
      const float sc = c < ni ? row[c] : 0.f;
      const bool tie = c <= s_col && ordered(sc) == t32;
      const unsigned long long m_tie = __ballot(tie);
      const unsigned int rank = seen + __popcll(m_tie & ((1ull << tid) - 1ull)) + 1;
      if (tie && rank > e) {
        unsigned int slot = atomicAdd(sh_count, 1u);
        if (slot < (unsigned)kpad) cand[slot] = make_key(sc, c);
      }
      seen += __popcll(m_tie);
    }
  }
}

// List form: writes the best k of a candidate list sorted by (score desc, column desc) that holds EVERY surviving entry >= the
// k-th score (the callers guarantee it: their thresholds are lower bounds of the k-th score), ties at the k-th score included.
template <int BLOCK>
__device__ void write_best_k(const uint64_t *cand, unsigned int n_c, int k, int q, int32_t *__restrict__ out_ids,
                             float *__restrict__ out_dist, int out_stride, int *__restrict__ fallback, float unscale_q) {
  const int tid = threadIdx.x;
  const uint32_t t32 = (uint32_t)(cand[k - 1] >> 32);
  const bool tie = (int)n_c > k && t32 == (uint32_t)(cand[k] >> 32);
  if (!tie) {
    if (tid == 0) fallback[q] = 0;
    for (int i = tid; i < k; i += BLOCK) {
      uint64_t key = cand[i];
      out_ids[(size_t)q * out_stride + i] = key_id(key);
      out_dist[(size_t)q * out_stride + i] = key_score(key) * unscale_q;
    }
    return;
  }
  // Exact tie at the k-th score t: the rule above.  The list is sorted by (score desc, column desc), i.e. [0, g) are the
  // entries > t and [g, g + m) the ties, highest column first; every entry >= t is in it (t >= tau).
  __shared__ unsigned int sh_g, sh_m, sh_e, sh_above;
  __shared__ int sh_s;
  if (tid == 0) sh_g = sh_m = sh_e = sh_above = 0;
  __syncthreads();
  for (int i = tid; i < (int)n_c; i += BLOCK) {
    const uint32_t key32 = (uint32_t)(cand[i] >> 32);
    if (key32 > t32) atomicAdd(&sh_g, 1u);
    else if (key32 == t32) atomicAdd(&sh_m, 1u);
  }
  __syncthreads();
  const int g = (int)sh_g, m = (int)sh_m, ng = g + m;
  if (ng > 1024) {  // thousands of tied entries: the quadratic rank below is not worth it, the materialising path takes the row
    if (tid == 0) fallback[q] = 1;
    return;
  }
  for (int i = tid; i < ng; i += BLOCK) {  // rank in ascending column order; rank k-1 is the saturation column
    const uint32_t col = (uint32_t)cand[i];
    int rank = 0;
    for (int j = 0; j < ng; ++j) rank += (uint32_t)cand[j] < col;
    if (rank == k - 1) sh_s = (int)col;
  }
  __syncthreads();
  const uint32_t s_col = (uint32_t)sh_s;
  for (int i = tid; i < ng; i += BLOCK) {
    const uint32_t col = (uint32_t)cand[i];
    if (i < g && col > s_col) atomicAdd(&sh_e, 1u);      // later arrivals above t: each evicts the lowest tied column
    if (i >= g && col > s_col) atomicAdd(&sh_above, 1u);  // ties that arrived after saturation never entered
  }
  __syncthreads();
  const int i0 = g + (int)sh_above, i1 = g + m - (int)sh_e;  // surviving ties: [i0, i1) -- columns <= s minus the e lowest
  if (tid == 0) fallback[q] = (g + (i1 - i0) == k) ? 0 : 1;   // always k by construction; anything else -> the exact path
  for (int i = tid; i < ng; i += BLOCK) {
    int slot = -1;
    if (i < g) slot = i;
    else if (i >= i0 && i < i1) slot = g + (i - i0);
    if (slot >= 0 && slot < k) {
      const uint64_t key = cand[i];
      out_ids[(size_t)q * out_stride + slot] = key_id(key);
      out_dist[(size_t)q * out_stride + slot] = key_score(key) * unscale_q;
    }
  }
}

// One workgroup per query row.  `cand` = k 64-bit slots (LDS when it fits, else global scratch).
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void select_kernel(const float *__restrict__ S, int ni, int k, int kpad,
                                                       int32_t *__restrict__ out_ids, float *__restrict__ out_dist,
                                                       int out_stride, uint64_t *__restrict__ global_cand, int use_lds,
                                                       const int *__restrict__ only_flagged) {
  if (only_flagged && !only_flagged[blockIdx.x]) return;  // rows already finished by select_pruned_kernel
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __shared__ unsigned int hist[256];
  __shared__ unsigned int sh_bucket, sh_remaining, sh_count;
  uint64_t *cand = use_lds ? reinterpret_cast<uint64_t *>(smem_raw) : global_cand + (size_t)blockIdx.x * kpad;
  const float *row = S + (size_t)blockIdx.x * ni;
  const int tid = threadIdx.x;

  uint64_t prefix = 0, mask = 0;
  unsigned int remaining = k;  // k <= ni guaranteed by the host
  bool ambiguous = false;      // more keys tie with the k-th SCORE than there are places left
  auto keys = [&](auto &&body) {
    for (int i = tid; i < ni; i += BLOCK) body(make_key(row[i], i));
  };
  for (int digit = 7; digit >= 4; --digit) {  // the four score bytes of the key
    if (radix_select_digit<BLOCK, uint64_t>(keys, digit * 8, prefix, mask, remaining, hist, &sh_bucket, &sh_remaining, &sh_count))
      break;  // boundary bucket taken entirely: no finer digits needed
    if (digit == 4) ambiguous = true;
  }

  if (tid == 0) sh_count = 0;
  for (int i = tid; i < kpad; i += BLOCK) cand[i] = 0;  // pads sort last
  __syncthreads();
  if (!ambiguous) {
    // (key & mask) >= prefix selects exactly k keys
    keys([&](uint64_t key) {
      if ((key & mask) >= prefix) {
        unsigned int slot = atomicAdd(&sh_count, 1u);
        if (slot < (unsigned)kpad) cand[slot] = key;
      }
    });
  } else {
    select_row_ties<BLOCK>(row, ni, k, kpad, (uint32_t)(prefix >> 32), cand, &sh_count);
  }
  __syncthreads();
  block_sort_desc<BLOCK>(cand, kpad);
  for (int i = tid; i < k; i += BLOCK) {
    uint64_t key = cand[i];
    out_ids[(size_t)blockIdx.x * out_stride + i] = key_id(key);
    out_dist[(size_t)blockIdx.x * out_stride + i] = key_score(key);
  }
}

// Pruned select: tau = the k-th largest tile maximum (maxima refreshed after the filters) is a lower bound of the k-th
// best surviving score: k distinct tiles each hold a surviving score >= tau.
// The tiles whose maximum reaches tau (about m of them) are scanned for scores >= tau (tens to a few hundred), which
// go to LDS; a bitonic sort orders them and the best k are written.  Rows that overflow the candidate buffer or have too few tiles raise `fallback[row]` and are redone by
// select_kernel; an exact tie at the k-th score is resolved inside the list (write_best_k: every entry >= the k-th score is in it).
constexpr int kCandCap = 4096;  // 32 KiB of LDS; heavy users (many liked items lower tau) need the headroom

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void select_pruned_kernel(const float *__restrict__ S, const float *__restrict__ tile_max,
                                                              int ni, int n_tiles, int k, int extra,
                                                              const int *__restrict__ filter_counts,
                                                              int32_t *__restrict__ out_ids, float *__restrict__ out_dist,
                                                              int out_stride, int *__restrict__ fallback) {
  __shared__ uint64_t cand[kCandCap];
  __shared__ unsigned int hist[256];
  __shared__ unsigned int sh_bucket, sh_remaining, sh_count;
  const int tid = threadIdx.x;
  const int q = blockIdx.x;
  const float *row = S + (size_t)q * ni;
  const float *tm = tile_max + (size_t)q * n_tiles;
  const int m = k + extra + (filter_counts ? filter_counts[q] : 0);
  if (m > n_tiles || k > kCandCap) {  // uniform
    if (tid == 0) fallback[q] = 1;
    return;
  }
  // m-th largest tile maximum.  Up to kRankTiles maxima (26 744 items: 418): by COUNTING -- the keys go to LDS (the upper half of
  // the candidate buffer, free until the scan below), every thread counts the keys greater than each of its own (index breaks
  // ties), the key with m - 1 greater ones is tau: one barrier instead of four histogram passes whose LDS atomics all land in
  // the two or three bins a row's maxima share (0.072 -> 0.02 ms per 1000 rows at configs[4]'s similar_items shape).  Beyond
  // that: 4-pass byte radix select over the (L2-resident) maxima (kth_largest_key)
  constexpr int kRankTiles = 1024;
  uint32_t tau;  // exact key of the m-th largest maximum
  if (n_tiles <= kRankTiles) {
    uint32_t *keys = reinterpret_cast<uint32_t *>(cand + kCandCap / 2);
    for (int i = tid; i < n_tiles; i += BLOCK) keys[i] = ordered(tm[i]);
    __syncthreads();
    for (int i = tid; i < n_tiles; i += BLOCK) {
      const uint32_t key = keys[i];
      int greater = 0;
      for (int j = 0; j < n_tiles; ++j) {
        const uint32_t o = keys[j];
        greater += (o > key) || (o == key && j < i);
      }
      if (greater == m - 1) sh_bucket = key;
    }
    __syncthreads();
    tau = sh_bucket;
    __syncthreads();  // (everybody has read tau and the keys: the candidate scan may overwrite them)
  } else {
    tau = kth_largest_key<BLOCK>(tm, n_tiles, (unsigned)m, hist, &sh_bucket, &sh_remaining);
  }

  if (tid == 0) sh_count = 0;
  __syncthreads();
  // every score >= tau lives in a tile whose maximum is >= tau (the maxima are exact: the GEMM epilogue writes them
  // and the filter kernels refresh the tiles they touch), so only those tiles -- about m of the n_tiles -- are read
  // from the score row.  The hit tiles are listed first (LDS, the upper half of the candidate buffer) and their scores then
  // read by ALL threads with four independent loads per trip: one tile per wavefront and step (the first form) was a chain of
  // a dozen dependent round trips to the freshly written score row per wavefront
  {
    uint32_t *hit = reinterpret_cast<uint32_t *>(cand + kCandCap / 2);  // [<= n_tiles] (n_tiles <= 2 kCandCap: checked below)
    __shared__ unsigned int sh_hits;
    if (tid == 0) sh_hits = 0;
    __syncthreads();
    const bool listed = n_tiles <= kCandCap;  // (4 bytes per tile in a 16 KB half buffer)
    if (listed) {
      for (int t = tid; t < n_tiles; t += BLOCK)
        if (ordered(tm[t]) >= tau) hit[atomicAdd(&sh_hits, 1u)] = (uint32_t)t;
      __syncthreads();
      const unsigned int n_hit = sh_hits;
      // the list and the candidates share the buffer: candidates go to the lower half only while the list is being read
      // (more than kCandCap / 2 of them: the row overflows -> fallback, as a full buffer would)
      const unsigned int total = n_hit * kTileItems;
      for (unsigned int base = tid; base < total; base += 4 * BLOCK) {
        float sc[4];
        int item[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const unsigned int idx = base + u * BLOCK;
          item[u] = idx < total ? (int)(hit[idx / kTileItems] * kTileItems + idx % kTileItems) : ni;
          sc[u] = item[u] < ni ? row[item[u]] : -FLT_MAX;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (item[u] < ni && ordered(sc[u]) >= tau) {
            unsigned int slot = atomicAdd(&sh_count, 1u);
            if (slot < (unsigned)kCandCap / 2) cand[slot] = make_key(sc[u], item[u]);
          }
        }
      }
      __syncthreads();
      if (sh_count > (unsigned)kCandCap / 2) {  // uniform
        if (tid == 0) fallback[q] = 1;
        return;
      }
    } else {
      const int lane = tid & 63, wave = tid >> 6;
      for (int base = wave * 64; base < n_tiles; base += (BLOCK / 64) * 64) {
        const int t = base + lane;
        unsigned long long hits = __ballot(t < n_tiles && ordered(tm[t]) >= tau);
        while (hits) {
          const int item = (base + __builtin_ctzll(hits)) * kTileItems + lane;
          hits &= hits - 1;
          if (item < ni) {
            const float sc = row[item];
            if (ordered(sc) >= tau) {
              unsigned int slot = atomicAdd(&sh_count, 1u);
              if (slot < (unsigned)kCandCap) cand[slot] = make_key(sc, item);
            }
          }
        }
      }
    }
  }
  __syncthreads();
  const unsigned int n_c = sh_count;
  if (n_c > (unsigned)kCandCap || n_c < (unsigned)k) {
    if (tid == 0) fallback[q] = 1;
    return;
  }
  if (n_c <= 256u) {  // short list: ordered by counting (distinct keys: the column is part of them), one barrier
    uint64_t *sorted = cand + kCandCap / 2;
    block_rank_sort<BLOCK>(cand, sorted, (int)n_c);
    write_best_k<BLOCK>(sorted, n_c, k, q, out_ids, out_dist, out_stride, fallback, 1.0f);
    return;
  }
  int npad = 2;
  while (npad < (int)n_c) npad <<= 1;
  for (int i = n_c + tid; i < npad; i += BLOCK) cand[i] = 0;
  __syncthreads();
  block_sort_desc<BLOCK>(cand, npad);
  write_best_k<BLOCK>(cand, n_c, k, q, out_ids, out_dist, out_stride, fallback, 1.0f);
}

// ---- emit path (the route is described in topk.hip): thresholds from the pre-pass subset, then the candidate lists -------------
constexpr int kEmitCap = 4096;  // candidates per query (32 KiB: the LDS sort buffer of select_candidates_kernel)

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void subset_threshold_kernel(const float *__restrict__ S_sub, int sub_cols, int k,
                                                                 uint32_t *__restrict__ tau, unsigned int *__restrict__ count) {
  __shared__ unsigned int hist[256];
  __shared__ unsigned int sh_bucket, sh_remaining;
  const int q = blockIdx.x;
  const uint32_t key = kth_largest_key<BLOCK>(S_sub + (size_t)q * sub_cols, sub_cols, (unsigned)min(k, sub_cols), hist, &sh_bucket,
                                              &sh_remaining);
  if (threadIdx.x == 0) {
    tau[q] = key;  // ordered(-FLT_MAX) when fewer than k subset entries survive the filters: everything is emitted -> fallback
    count[q] = 0;
  }
}

// Small k (the recommend() case, k = 10).  The threshold only has to be a LOWER BOUND of the row's k-th best score, so the
// subset's exact k-th largest entry is not needed: every thread keeps the maximum of the entries it scanned (BLOCK disjoint
// groups) and tau = the k-th largest of those BLOCK maxima -- k distinct entries of the subset reach it.  With 256 groups and
// k = 10 it is the subset's exact k-th largest in 84 % of the rows and its (k+1)-th or (k+2)-th otherwise (a few more candidates).
// Each wavefront takes its k largest lane maxima out by DPP rounds (no LDS, no barrier), wavefront 0 merges the 4 x k survivors:
// ONE barrier per row instead of one per round with a rescan of 24 registers (round 3's exact form: 23 us per 1000 queries).
// Filtered entries carry ordered(-FLT_MAX); a row with fewer than k live groups gets that as tau: everything is emitted -> fallback.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void subset_threshold_groupmax_kernel(const float *__restrict__ S_sub, int sub_cols, int k,
                                                                          uint32_t *__restrict__ tau, unsigned int *__restrict__ count) {
  constexpr int WAVES = BLOCK / 64;
  static_assert(WAVES * 32 <= 128, "the merge holds two values per lane");
  __shared__ uint32_t part[WAVES * 32];
  const int tid = threadIdx.x, q = blockIdx.x, lane = tid & 63, wave = tid >> 6;
  const float *v = S_sub + (size_t)q * sub_cols;
  const uint32_t floor_key = ordered(-FLT_MAX);
  uint32_t m = floor_key;  // an empty group counts as filtered
  for (int i = tid; i < sub_cols; i += BLOCK) m = max(m, ordered(v[i]));
  const int rounds = min(k, 32);
  uint32_t mine = 0u;  // lane `it` of a wavefront ends with the wavefront's it-th largest group maximum; 0 = taken / none
  for (int it = 0; it < rounds; ++it) {
    const uint32_t top = wave_allmax_u32(m);
    if (lane == it) mine = top;
    const unsigned long long holders = __ballot(m == top);
    if (lane == (int)__builtin_ctzll(holders)) m = 0u;
  }
  if (lane < 32) part[wave * 32 + lane] = lane < rounds ? mine : 0u;
  __syncthreads();
  if (wave == 0) {
    uint32_t a = part[lane], b = part[64 + lane];
    uint32_t kth = 0u;
    for (int it = 0; it < rounds; ++it) {
      const uint32_t lm = max(a, b);
      kth = wave_allmax_u32(lm);
      const unsigned long long holders = __ballot(lm == kth);
      if (lane == (int)__builtin_ctzll(holders)) {
        if (a == kth) a = 0u;
        else b = 0u;
      }
    }
    if (lane == 0) {
      tau[q] = max(kth, floor_key);
      count[q] = 0;
    }
  }
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void select_candidates_kernel(const uint64_t *__restrict__ gcand, const unsigned int *__restrict__ count,
                                                                  int cap, int k, int32_t *__restrict__ out_ids,
                                                                  float *__restrict__ out_dist, int out_stride,
                                                                  int *__restrict__ fallback, const float *__restrict__ row_unscale) {
  __shared__ uint64_t cand[kEmitCap];
  const int tid = threadIdx.x, q = blockIdx.x;
  const float unscale_q = row_unscale ? row_unscale[q] : 1.f;  // (a power of two: exact)
  const unsigned int n_c = count[q];
  if (n_c > (unsigned)cap || n_c < (unsigned)k) {  // uniform
    if (tid == 0) fallback[q] = 1;
    return;
  }
  int npad = 2;
  while (npad < (int)n_c) npad <<= 1;
  for (int i = tid; i < npad; i += BLOCK) cand[i] = i < (int)n_c ? gcand[(size_t)q * cap + i] : 0;  // pads sort last
  __syncthreads();
  block_sort_desc<BLOCK>(cand, npad);
  if ((uint32_t)(cand[0] >> 32) >= 0xFF800000u) {  // best candidate +inf / NaN (uniform): an operand left the fp16 form's range
    if (tid == 0) fallback[q] = 1;                 // (or the scores really are infinite) -- the exact path decides
    return;
  }
  write_best_k<BLOCK>(cand, n_c, k, q, out_ids, out_dist, out_stride, fallback, unscale_q);
}

// Candidates of the SCREENED emit pass (topk_resident.h MODE 3): the keys carry one-product accumulators, each within eps_q of the
// row's scaled exact score.  Sort by them; with A_k the k-th largest, every entry whose exact score reaches the k-th EXACT score
// has an accumulator >= A_k - 2 eps_q (k entries have exact scores >= A_k - eps_q, so the k-th exact score is at least that; an
// entry that reaches it lies at most eps_q below in the approximate order).  Those R entries -- k plus a handful -- are re-scored
// from the stored factors in fp32 (one wavefront per entry, the reference's own arithmetic: an fp32 dot product of the row and
// the item, implicit/gpu/knn.cu:131-147 / cpu/topk.pyx:45-47), ordered by (score desc, column desc) and written with the heap's
// tie rule.  More than kScreenCap of them (eps_q is a worst-case bound: tiny queries against a catalogue with huge outliers) or a
// non-finite score: the row goes to the exact path.
constexpr int kScreenCap = 1024;
#ifdef RQ_SCREEN_STATS  // variant builds: rows, candidates, re-scored entries of the screened select
__device__ unsigned long long rq_screen_stats[4];
#endif
template <int BLOCK, typename TQs, typename TIs>
__global__ __launch_bounds__(BLOCK) void select_screened_kernel(const uint64_t *__restrict__ gcand, const unsigned int *__restrict__ count,
                                                                int cap, int k, int32_t *__restrict__ out_ids, float *__restrict__ out_dist,
                                                                int out_stride, int *__restrict__ fallback, const float *__restrict__ row_eps,
                                                                const TQs *__restrict__ Q, const TIs *__restrict__ I, int f,
                                                                int *__restrict__ n_out) {
  __shared__ uint64_t cand[kEmitCap];
  __shared__ unsigned int sh_r;
  const int tid = threadIdx.x, q = blockIdx.x;
  const unsigned int n_c = count[q];
  if (tid == 0) n_out[q] = (int)min(n_c, (unsigned)cap + 1u);
  if (n_c > (unsigned)cap || n_c < (unsigned)k) {  // uniform
    if (tid == 0) fallback[q] = 1;
    return;
  }
  // the query row's share of this lane (EIGHT lanes per re-scored entry, four consecutive factors per lane and trip; f <= 256:
  // the resident form's limit), requested before anything else: its latency runs under the sort
  const int g = tid & 7;
  float4 qv[8];  // (f is a multiple of 8 on this path: whole 4-factor pieces, one vector load each)
  {
    const TQs *qrow = Q + (size_t)q * f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = 4 * g + 32 * j;
      qv[j] = c < f ? load4(qrow + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  int npad = 2;
  while (npad < (int)n_c) npad <<= 1;
  for (int i = tid; i < npad; i += BLOCK) cand[i] = i < (int)n_c ? gcand[(size_t)q * cap + i] : 0;  // pads sort last
  if (tid == 0) sh_r = 0;
  __syncthreads();
  // short lists (the usual case: a few dozen entries) are ordered by counting -- one barrier instead of the bitonic network's
  // log^2 n; beyond kRankSort entries the quadratic count loses to the network
  constexpr int kRankSort = 128;
  uint64_t *lst = cand;
  if (n_c <= (unsigned)kRankSort) {
    lst = cand + 2048;
    block_rank_sort<BLOCK>(cand, lst, (int)n_c);
  } else {
    block_sort_desc<BLOCK>(cand, npad);
  }
  const float eps = row_eps[q];
  const float a_k = key_score(lst[k - 1]);
  const float cut = a_k - 2.f * eps;
  if (!(eps >= 0.f) || !(eps <= FLT_MAX) || !(a_k == a_k) || (uint32_t)(lst[0] >> 32) >= 0xFF800000u) {  // (uniform) NaN / inf somewhere
    if (tid == 0) fallback[q] = 1;
    return;
  }
  // R = entries with an accumulator >= cut: a prefix of the sorted list
  for (int i = tid; i < (int)n_c; i += BLOCK)
    if (key_score(lst[i]) >= cut) atomicMax(&sh_r, (unsigned)i + 1u);
  __syncthreads();
  const int n_r = (int)sh_r;
#ifdef RQ_SCREEN_STATS
  if (tid == 0) atomicAdd(&rq_screen_stats[0], 1ull), atomicAdd(&rq_screen_stats[1], (unsigned long long)n_c), atomicAdd(&rq_screen_stats[2], (unsigned long long)n_r), atomicMax(&rq_screen_stats[3], (unsigned long long)n_r);
#endif
  if (n_r > kScreenCap) {  // uniform
    if (tid == 0) fallback[q] = 1;
    return;
  }
  // exact scores of the R entries.  Nearly every row re-scores k plus one or two, but a row whose scores are all small against its
  // bound re-scores hundreds (624 seen on the bench's trained factors) and the launch lasts as long as its slowest row: eight
  // lanes per entry and two entries per group and trip = 128 gathers of a row in flight; fixed-order sum over the group
  bool bad = false;
  constexpr int PER = BLOCK / 8;
  for (int i0 = tid >> 3; i0 < n_r; i0 += 2 * PER) {
    const int i1 = i0 + PER;
    const bool two = i1 < n_r;
    const int item0 = key_id(lst[i0]), item1 = two ? key_id(lst[i1]) : item0;
#ifdef RQ_SCREEN_KO  // (timing only) 1: no gathers -- every entry reads item row 0;  2: no re-scoring at all
    const TIs *r0 = I + (size_t)((RQ_SCREEN_KO & 1) ? 0 : item0) * f, *r1 = I + (size_t)((RQ_SCREEN_KO & 1) ? 0 : item1) * f;
    if (RQ_SCREEN_KO & 2) break;
#else
    const TIs *r0 = I + (size_t)item0 * f, *r1 = I + (size_t)item1 * f;
#endif
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = 4 * g + 32 * j;
      if (c < f) {
        const float4 y0 = load4(r0 + c), y1 = load4(r1 + c);
        s0 = fmaf(qv[j].x, y0.x, s0), s0 = fmaf(qv[j].y, y0.y, s0), s0 = fmaf(qv[j].z, y0.z, s0), s0 = fmaf(qv[j].w, y0.w, s0);
        s1 = fmaf(qv[j].x, y1.x, s1), s1 = fmaf(qv[j].y, y1.y, s1), s1 = fmaf(qv[j].z, y1.z, s1), s1 = fmaf(qv[j].w, y1.w, s1);
      }
    }
    s0 += __shfl_xor(s0, 4, 64), s0 += __shfl_xor(s0, 2, 64), s0 += __shfl_xor(s0, 1, 64);
    s1 += __shfl_xor(s1, 4, 64), s1 += __shfl_xor(s1, 2, 64), s1 += __shfl_xor(s1, 1, 64);
    if (!(fabsf(s0) <= FLT_MAX) || !(fabsf(s1) <= FLT_MAX)) bad = true;
    if (g == 0) {
      lst[i0] = make_key(s0, item0);
      if (two) lst[i1] = make_key(s1, item1);
    }
  }
  if (__syncthreads_or(bad)) {
    if (tid == 0) fallback[q] = 1;
    return;
  }
  uint64_t *fin = lst;
  if (n_r <= kRankSort) {
    fin = lst == cand ? cand + 2048 : cand;  // (the two regions do not overlap)
    block_rank_sort<BLOCK>(lst, fin, n_r);
  } else {  // (n_r <= kScreenCap = 1024: the pads stay inside the list's 2048-entry region)
    int rpad = 2;
    while (rpad < n_r) rpad <<= 1;
    for (int i = n_r + tid; i < rpad; i += BLOCK) lst[i] = 0;
    __syncthreads();
    block_sort_desc<BLOCK>(lst, rpad);
  }
  write_best_k<BLOCK>(fin, (unsigned)n_r, k, q, out_ids, out_dist, out_stride, fallback, 1.f);
}

}  // namespace imp
#endif  // IMPLICIT_AMD_CSRC_TOPK_SELECT_H_
