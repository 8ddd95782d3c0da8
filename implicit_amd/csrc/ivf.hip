// IVF-Flat: a native approximate-nearest-neighbour index over the rows of a factor matrix.
//
// The reference wraps faiss's GpuIndexIVFFlat (implicit/ann/faiss.py); nothing of that stack exists here, so this is the
// structure itself: a spherical k-means quantiser of `nlist` centroids, the vectors copied list by list (one contiguous
// range per list, ascending ids inside it), and a search that scans only the `nprobe` lists nearest a query by inner product.
//
// Everything is fp32 (fp16 input is widened), rows are zero-padded to f_pad = 4 * ceil(f / 4) floats, and everything is
// deterministic: the same inputs give the same bits.
//
// One GEMM kernel serves all three products (vector x centroid of the k-means assignment, query x centroid of the coarse
// step, query x list vector of the scan).  ivf_scan_kernel runs over (list, tile of 64 of the queries that probe that list,
// tile of 128 of its vectors): a list is read ONCE PER QUERY TILE and scored as a small GEMM on v_mfma_f32_32x32x2_f32,
// not once per (query, list) pair.  The dense products are the same kernel over one "list" holding every centroid, probed
// by every row.  The fp32-input MFMA is an exact k-ordered fmaf chain and the k order is the same in every tile, so a score
// depends only on its (query, vector) pair and never on where either sits in a tile: duplicate vectors score bit-identically.
//
// Grouping (ivf_group): a stable counting sort by a small key, used for vectors by list (the inverted lists) and for
// (query, probe) pairs by list (the scan's query groups).  The elements are cut into runs, one wavefront each: a histogram
// per run, an exclusive scan per key over the runs and over the keys, and a scatter in which the wavefront walks its run in
// element order.  The only atomics are integer counts (whose result does not depend on arrival order) and, in the scatter,
// adds to counters that exactly one wavefront touches in program order; the layout never depends on timing.
//
// Selection (ivf_select_kernel): one workgroup per query over that query's score segments, keys ordered(score) << 32 | id.
// A histogram of the top 11 key bits isolates the far tail that holds the k best, which is copied to LDS; an MSB-first radix
// select of the k-th largest key, a gather of the winners and a bitonic sort follow there: the total order (score desc, id
// desc) of imp_knn_topk.  Ids are unique within a query's candidates, so keys are, and the select is exact.
//
// A search keeps every score of a chunk of queries in one buffer (a segment per (query, probe) pair); queries are taken in
// chunks that keep it within the budget of KnnQuery, min(free / 2, 4 GiB).
#include <hip/hip_fp16.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <functional>

#include "common.h"
#include "select_ops.h"  // the score/id key (make_key, key_id, key_score), block_sort_desc

struct imp_ivf {
  size_t n = 0, f = 0;
  int f_pad = 0, nlist = 0;
  size_t budget = 0;                    // bytes of temporaries of one search chunk / one assignment chunk
  imp::DeviceArray<float> centroids;    // nlist x f_pad, unit rows (or zero)
  imp::DeviceArray<int32_t> list_off;   // nlist + 1
  imp::DeviceArray<int32_t> list_ids;   // n: original row ids, ascending inside a list
  imp::DeviceArray<float> list_vecs;    // n x f_pad, row p = vector list_ids[p]
  std::vector<int64_t> lens_desc_sum;   // host: [i] = the sum of the i longest lists' lengths (nlist + 1 entries)
  // temporaries of a search, kept between calls and grown on demand (an allocation of gigabytes costs more than a search);
  // imp_ivf_set_temp_memory drops them
  struct Workspace {
    imp::DeviceArray<float> Q, S, probe_dist, out_dist;
    imp::DeviceArray<int32_t> probes, sorted, inv, pair_off, out_ids;
    imp::DeviceArray<unsigned> group_cnt;
  } ws;
};

namespace imp {

typedef float ivf_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kIvfBM = 64;    // queries per tile
constexpr int kIvfBN = 128;   // vectors per tile
constexpr int kIvfBK = 32;    // factors per K step
constexpr int kIvfLd = kIvfBK + 1;
constexpr int kIvfMaxK = 1024;
constexpr int kIvfRun = 1024;             // elements per run of the grouping, at least
constexpr int64_t kIvfMaxCounters = (int64_t)1 << 24;  // runs x keys of the grouping's counter table, at most

__device__ __forceinline__ uint64_t ivf_max64(uint64_t a, uint64_t b) { return a < b ? b : a; }
__device__ __forceinline__ int64_t ivf_min64(int64_t a, int64_t b) { return a < b ? a : b; }

// ---- centroids (the padded copies are pad_rows', common.h) ---------------------------------------------------------------
// sum of squares of row[0 .. f_pad) over the 256 threads of a workgroup, in a fixed tree; `red` holds 256 floats
__device__ float ivf_block_sumsq(const float *row, int f_pad, float *red) {
  float s = 0.f;
  for (int d = threadIdx.x; d < f_pad; d += 256) s = fmaf(row[d], row[d], s);
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

// centroid c = the unit-normalised row init_rows[c]; a zero row stays zero
__global__ __launch_bounds__(256) void ivf_init_centroids_kernel(const float *__restrict__ vec, const int32_t *__restrict__ init_rows,
                                                                 int f_pad, float *__restrict__ cent) {
  __shared__ float red[256];
  const float *row = vec + (size_t)init_rows[blockIdx.x] * f_pad;
  const float s = ivf_block_sumsq(row, f_pad, red);
  const bool ok = s > 0.f && s <= FLT_MAX;
  const float norm = sqrtf(s);
  for (int d = threadIdx.x; d < f_pad; d += 256) cent[(size_t)blockIdx.x * f_pad + d] = ok ? row[d] / norm : 0.f;
}

// centroid l = the normalised mean of its list, summed in ascending vector id; an empty list or a zero mean keeps the old one
__global__ __launch_bounds__(256) void ivf_update_centroids_kernel(const float *__restrict__ vec, const int32_t *__restrict__ list_off,
                                                                   const int32_t *__restrict__ list_ids, int f_pad,
                                                                   float *__restrict__ cent) {
  __shared__ float red[256];
  __shared__ float mean[1024];
  const int b = list_off[blockIdx.x], e = list_off[blockIdx.x + 1];
  if (e == b) return;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i = b; i < e; ++i) {
    const float *row = vec + (size_t)list_ids[i] * f_pad;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int d = threadIdx.x + 256 * j;
      if (d < f_pad) acc[j] += row[d];
    }
  }
  const float count = (float)(e - b);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int d = threadIdx.x + 256 * j;
    if (d < f_pad) mean[d] = acc[j] / count;
  }
  __syncthreads();
  const float s = ivf_block_sumsq(mean, f_pad, red);
  if (!(s > 0.f && s <= FLT_MAX)) return;
  const float norm = sqrtf(s);
  for (int d = threadIdx.x; d < f_pad; d += 256) cent[(size_t)blockIdx.x * f_pad + d] = mean[d] / norm;
}

__global__ void ivf_gather_rows_kernel(const float *__restrict__ vec, const int32_t *__restrict__ list_ids, size_t n, int f_pad,
                                       float *__restrict__ out) {
  const int f4 = f_pad >> 2;
  const size_t total = n * (size_t)f4;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t p = i / f4;
    const int c = (int)(i - p * f4);
    reinterpret_cast<float4 *>(out)[i] = reinterpret_cast<const float4 *>(vec + (size_t)list_ids[p] * f_pad)[c];
  }
}

// ---- the grouped GEMM --------------------------------------------------------------------------------------------------
// Lists l = 0 .. nlist - 1: rows [list_off[l], list_off[l + 1]) of V, probed by the pairs [pair_off[l], pair_off[l + 1]) of the
// grouped order; pair p belongs to row sorted[p] / nprobe of Q (sorted == nullptr: row p).  Its scores go to
// S[score_base[l] + (p - pair_off[l]) * len(l) + v], v the vector's place in the list.  tile_off[l]: the first of the list's
// ceil(pairs / 64) * ceil(len / 128) tiles; consecutive tiles walk one list under one query tile.
struct IvfScanArgs {
  const float *Q, *V;
  float *S;
  const int32_t *list_off, *pair_off, *sorted, *tile_off;
  const int64_t *score_base;
  int nlist, nprobe, f_pad;
};

__global__ __launch_bounds__(256) void ivf_scan_kernel(const IvfScanArgs a) {
  __shared__ float Qs[kIvfBM * kIvfLd];
  __shared__ float Vs[kIvfBN * kIvfLd];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int total = a.tile_off[a.nlist];
  for (int w = blockIdx.x; w < total; w += gridDim.x) {
    int lo = 0, hi = a.nlist;  // the last list whose first tile is <= w (lists without tiles share their successor's offset)
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (a.tile_off[mid] <= w) lo = mid; else hi = mid;
    }
    const int l = lo;
    const int v_begin = a.list_off[l], len = a.list_off[l + 1] - v_begin;
    const int p_begin = a.pair_off[l], np = a.pair_off[l + 1] - p_begin;
    const int nvt = (len + kIvfBN - 1) / kIvfBN;
    const int r = w - a.tile_off[l];
    const int q0 = (r / nvt) * kIvfBM, v0 = (r % nvt) * kIvfBN;
    int qrow[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int p = q0 + ((tid + 256 * i) >> 3);
      qrow[i] = p < np ? (a.sorted ? a.sorted[p_begin + p] / a.nprobe : p_begin + p) : -1;
    }
    ivf_f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;

    for (int k0 = 0; k0 < a.f_pad; k0 += kIvfBK) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int e = tid + 256 * i, row = e >> 3, c = (e & 7) * 4, k = k0 + c;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (qrow[i] >= 0 && k < a.f_pad) x = *reinterpret_cast<const float4 *>(a.Q + (size_t)qrow[i] * a.f_pad + k);
        float *d = Qs + row * kIvfLd + c;
        d[0] = x.x, d[1] = x.y, d[2] = x.z, d[3] = x.w;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int e = tid + 256 * i, row = e >> 3, c = (e & 7) * 4, k = k0 + c, v = v0 + row;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (v < len && k < a.f_pad) x = *reinterpret_cast<const float4 *>(a.V + (size_t)(v_begin + v) * a.f_pad + k);
        float *d = Vs + row * kIvfLd + c;
        d[0] = x.x, d[1] = x.y, d[2] = x.z, d[3] = x.w;
      }
      __syncthreads();
      // wave w: queries [0, 64) x vectors [32w, 32w + 32): two 32 x 32 tiles
      const int kh = lane >> 5, l31 = lane & 31;
#pragma unroll 8
      for (int kk = 0; kk < kIvfBK; kk += 2) {
        const float b = Vs[(32 * wave + l31) * kIvfLd + kk + kh];
        const float a0 = Qs[l31 * kIvfLd + kk + kh];
        const float a1 = Qs[(32 + l31) * kIvfLd + kk + kh];
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc[1], 0, 0, 0);
      }
      __syncthreads();
    }
    const int v = v0 + 32 * wave + (lane & 31);
    if (v < len) {
      float *out = a.S + a.score_base[l] + v;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int p = q0 + 32 * t + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
          if (p < np) out[(int64_t)p * len] = acc[t][e];
        }
    }
  }
}

// the one-list plan of a dense product: `cols` rows of V, probed by rows 0 .. rows - 1 of Q
__global__ void ivf_dense_plan_kernel(int rows, int cols, int32_t *list_off, int32_t *pair_off) {
  list_off[0] = 0, list_off[1] = cols, pair_off[0] = 0, pair_off[1] = rows;
}

// tile_off / score_base: exclusive scans over the lists of their tile and score counts (one workgroup)
__global__ __launch_bounds__(1024) void ivf_plan_kernel(const int32_t *__restrict__ list_off, const int32_t *__restrict__ pair_off,
                                                        int nlist, int32_t *__restrict__ tile_off, int64_t *__restrict__ score_base) {
  __shared__ int64_t st[1024], ss[1024];
  const int per = (nlist + 1023) / 1024, b = min(nlist, (int)threadIdx.x * per), e = min(nlist, b + per);
  int64_t t = 0, s = 0;
  for (int l = b; l < e; ++l) {
    const int64_t len = list_off[l + 1] - list_off[l], np = pair_off[l + 1] - pair_off[l];
    if (len > 0 && np > 0) t += ((np + kIvfBM - 1) / kIvfBM) * ((len + kIvfBN - 1) / kIvfBN), s += np * len;
  }
  st[threadIdx.x] = t, ss[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t rt = 0, rs = 0;
    for (int i = 0; i < 1024; ++i) {
      const int64_t ct = st[i], cs = ss[i];
      st[i] = rt, ss[i] = rs, rt += ct, rs += cs;
    }
    tile_off[nlist] = (int32_t)rt, score_base[nlist] = rs;
  }
  __syncthreads();
  t = st[threadIdx.x], s = ss[threadIdx.x];
  for (int l = b; l < e; ++l) {
    const int64_t len = list_off[l + 1] - list_off[l], np = pair_off[l + 1] - pair_off[l];
    tile_off[l] = (int32_t)t, score_base[l] = s;
    if (len > 0 && np > 0) t += ((np + kIvfBM - 1) / kIvfBM) * ((len + kIvfBN - 1) / kIvfBN), s += np * len;
  }
}

// ---- grouping: stable counting sort by key -----------------------------------------------------------------------------
// run r = elements [r * run, (r + 1) * run); cnt[r][key]
__global__ __launch_bounds__(64) void ivf_group_hist_kernel(const int32_t *__restrict__ keys, int64_t n, int run, int nkeys,
                                                            unsigned *__restrict__ cnt) {
  const int64_t b = (int64_t)blockIdx.x * run, e = ivf_min64(n, b + run);
  for (int64_t i = b + threadIdx.x; i < e; i += 64) atomicAdd(&cnt[(size_t)blockIdx.x * nkeys + keys[i]], 1u);
}

// per key: cnt[r][key] becomes the number of its elements in the runs before r; totals[key] the number in all of them
__global__ void ivf_group_colscan_kernel(unsigned *__restrict__ cnt, int nruns, int nkeys, int32_t *__restrict__ totals) {
  const int key = blockIdx.x * blockDim.x + threadIdx.x;
  if (key >= nkeys) return;
  unsigned run = 0;
  for (int r = 0; r < nruns; ++r) {
    const unsigned c = cnt[(size_t)r * nkeys + key];
    cnt[(size_t)r * nkeys + key] = run;
    run += c;
  }
  totals[key] = (int32_t)run;
}

// off[0 .. n] = exclusive scan of totals[0 .. n) (one workgroup)
__global__ __launch_bounds__(1024) void ivf_exclusive_scan_kernel(const int32_t *__restrict__ totals, int n, int32_t *__restrict__ off) {
  __shared__ int64_t st[1024];
  const int per = (n + 1023) / 1024, b = min(n, (int)threadIdx.x * per), e = min(n, b + per);
  int64_t t = 0;
  for (int i = b; i < e; ++i) t += totals[i];
  st[threadIdx.x] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t run = 0;
    for (int i = 0; i < 1024; ++i) {
      const int64_t c = st[i];
      st[i] = run, run += c;
    }
    off[n] = (int32_t)run;
  }
  __syncthreads();
  t = st[threadIdx.x];
  for (int i = b; i < e; ++i) off[i] = (int32_t)t, t += totals[i];
}

// One wavefront per run, walking it 64 elements at a time in element order.  A lane's place: the key's offset, plus the
// key's elements of earlier runs and earlier steps (cnt[run][key], which only this wavefront touches, advanced once per step
// by the first lane of every key), plus the lower lanes of this step that hold the same key.
__global__ __launch_bounds__(64) void ivf_group_scatter_kernel(const int32_t *__restrict__ keys, int64_t n, int run, int nkeys,
                                                               unsigned *__restrict__ cnt, const int32_t *__restrict__ off,
                                                               int32_t *__restrict__ order, int32_t *__restrict__ inv) {
  const int lane = threadIdx.x;
  const int64_t b = (int64_t)blockIdx.x * run, e = ivf_min64(n, b + run);
  for (int64_t i0 = b; i0 < e; i0 += 64) {
    const int64_t i = i0 + lane;
    const bool valid = i < e;
    const int key = valid ? keys[i] : -1;
    int rank = 0, count = 0, first = 64;
    for (int j = 0; j < 64; ++j) {
      const int kj = __shfl(key, j);
      const bool same = kj == key;
      rank += (same && j < lane) ? 1 : 0;
      count += same ? 1 : 0;
      if (same && first == 64) first = j;
    }
    unsigned base = 0;
    if (valid && rank == 0) base = atomicAdd(&cnt[(size_t)blockIdx.x * nkeys + key], (unsigned)count);
    base = __shfl(base, first);
    if (valid) {
      const int32_t pos = off[key] + (int32_t)base + rank;
      order[pos] = (int32_t)i;
      if (inv) inv[i] = pos;
    }
  }
}

// ---- selection ---------------------------------------------------------------------------------------------------------
// out[row] = the column of the best key of row `row` of the dense score matrix S (rows x ncol): one wavefront per row
__global__ __launch_bounds__(256) void ivf_argmax_kernel(const float *__restrict__ S, int64_t rows, int ncol, int32_t *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  uint64_t best = 0;
  for (int c = lane; c < ncol; c += 64) best = ivf_max64(best, make_key(S[row * ncol + c], c));
  for (int m = 32; m > 0; m >>= 1) {
    const uint32_t hi = __shfl_xor((uint32_t)(best >> 32), m), lo = __shfl_xor((uint32_t)best, m);
    best = ivf_max64(best, ((uint64_t)hi << 32) | lo);
  }
  if (lane == 0) out[row] = key_id(best);
}

// Candidates of query q.  Dense (probes == nullptr): S[q * ncand .. + ncand), id = column.  Grouped: for each of its P probes
// j, with l = probes[q * P + j] and p = inv[q * P + j] the pair's place in the grouped order, the len(l) scores at
// S[score_base[l] + (p - pair_off[l]) * len(l)], ids list_ids[list_off[l] ..].
struct IvfSelectArgs {
  const float *S;
  const int32_t *probes, *inv, *pair_off, *list_off, *list_ids;
  const int64_t *score_base;
  int P, ncand, k, kpad;
  int32_t *out_ids;
  float *out_dist;
};

template <typename F> __device__ __forceinline__ void ivf_for_each_candidate(const IvfSelectArgs &a, int64_t q, F &&body) {
  if (!a.probes) {
    const float *s = a.S + q * a.ncand;
    for (int v = threadIdx.x; v < a.ncand; v += 256) body(make_key(s[v], v));
    return;
  }
  for (int j = 0; j < a.P; ++j) {
    const int l = a.probes[q * a.P + j], p = a.inv[q * a.P + j];
    const int lb = a.list_off[l], len = a.list_off[l + 1] - lb;
    const float *s = a.S + a.score_base[l] + (int64_t)(p - a.pair_off[l]) * len;
    const int32_t *ids = a.list_ids + lb;
    for (int v = threadIdx.x; v < len; v += 256) body(make_key(s[v], ids[v]));
  }
}

// One workgroup per query.  Pass 1 histograms the top 11 bits of every key (sign, exponent, two mantissa bits) and finds the
// bucket the k-th best falls into; when that bucket and the ones above it hold at most kIvfSurvivors keys (the usual case:
// the k best are the far tail), pass 2 copies them to LDS and everything after reads LDS only -- two reads of the scores in
// all.  Otherwise the byte-wise radix select below walks the scores themselves.  Either way the winners are the `want` largest
// keys, found exactly, then sorted.
constexpr int kIvfSurvivors = 2048;

// All 256 threads: the bucket of hist[0 .. 256 * per) that holds the want-th largest key (1 <= want <= the keys counted).
// out[0] = that bucket, out[1] = the keys in the buckets above it, out[2] = the keys in it.  Thread t adds its `per`
// buckets, a suffix scan over the 256 sums finds the thread whose range holds the boundary, and that thread walks its range.
__device__ __forceinline__ void ivf_find_bucket(const unsigned *hist, int per, unsigned want, unsigned *scan, unsigned *out) {
  const int t = threadIdx.x;
  unsigned own = 0;
  for (int i = 0; i < per; ++i) own += hist[t * per + i];
  scan[t] = own;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const unsigned v = scan[t] + (t + off < 256 ? scan[t + off] : 0u);
    __syncthreads();
    scan[t] = v;
    __syncthreads();
  }
  unsigned above = scan[t] - own;
  if (above < want && want <= above + own) {
    int b = t * per + per - 1;
    for (; b > t * per; --b) {
      if (above + hist[b] >= want) break;
      above += hist[b];
    }
    out[0] = b, out[1] = above, out[2] = hist[b];
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void ivf_select_kernel(const IvfSelectArgs a) {
  __shared__ unsigned hist[2048];
  __shared__ uint64_t survivors[kIvfSurvivors];
  __shared__ uint64_t cand[kIvfMaxK];
  __shared__ unsigned scan[256];
  __shared__ unsigned found[3];
  __shared__ unsigned sh_count;
  const int tid = threadIdx.x;
  const int64_t q = blockIdx.x;
  int64_t total = a.ncand;
  if (a.probes) {
    total = 0;
    for (int j = 0; j < a.P; ++j) {
      const int l = a.probes[q * a.P + j];
      total += a.list_off[l + 1] - a.list_off[l];
    }
  }
  const unsigned want = (unsigned)ivf_min64(a.k, total);
  unsigned n_lds = 0;
  bool in_lds = false;
  if (total > a.k) {
    for (int i = tid; i < 2048; i += 256) hist[i] = 0;
    __syncthreads();
    ivf_for_each_candidate(a, q, [&](uint64_t key) { atomicAdd(&hist[key >> 53], 1u); });
    __syncthreads();
    ivf_find_bucket(hist, 8, want, scan, found);
    const unsigned first = found[0];
    n_lds = found[1] + found[2];
    __syncthreads();
    if (n_lds <= (unsigned)kIvfSurvivors) {
      if (tid == 0) sh_count = 0;
      __syncthreads();
      ivf_for_each_candidate(a, q, [&](uint64_t key) {
        if ((key >> 53) >= first) {
          const unsigned slot = atomicAdd(&sh_count, 1u);
          if (slot < (unsigned)kIvfSurvivors) survivors[slot] = key;
        }
      });
      __syncthreads();
      in_lds = true;
    }
  }
  auto each = [&](auto &&body) {
    if (in_lds) {
      for (unsigned i = tid; i < n_lds; i += 256) body(survivors[i]);
    } else {
      ivf_for_each_candidate(a, q, body);
    }
  };
  uint64_t thr = 0;  // every key >= thr is a winner: exactly `want` of them
  if (total > a.k) {
    uint64_t prefix = 0, mask = 0;
    unsigned remaining = want;
    for (int digit = 7; digit >= 0; --digit) {
      const int shift = digit * 8;
      hist[tid] = 0;
      __syncthreads();
      each([&](uint64_t key) {
        if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 0xFF], 1u);
      });
      __syncthreads();
      ivf_find_bucket(hist, 1, remaining, scan, found);
      prefix |= (uint64_t)found[0] << shift, mask |= (uint64_t)0xFF << shift;
      remaining -= found[1];
      const bool all = found[2] == remaining;
      __syncthreads();
      if (all) break;  // the boundary bucket is taken whole
    }
    thr = prefix;
  }
  if (tid == 0) sh_count = 0;
  __syncthreads();
  each([&](uint64_t key) {
    if (key >= thr) {
      const unsigned slot = atomicAdd(&sh_count, 1u);
      if (slot < (unsigned)a.kpad) cand[slot] = key;
    }
  });
  __syncthreads();
  for (int i = (int)want + tid; i < a.kpad; i += 256) cand[i] = 0;  // pads sort last
  __syncthreads();
  block_sort_desc<256>(cand, a.kpad);
  for (int i = tid; i < a.k; i += 256) {
    const bool filled = i < (int)want;
    a.out_ids[q * a.k + i] = filled ? key_id(cand[i]) : -1;
    a.out_dist[q * a.k + i] = filled ? key_score(cand[i]) : -FLT_MAX;
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
static size_t ivf_default_budget() {
  size_t free_b = 0, total_b = 0;
  IMP_CHECK_HIP(hipMemGetInfo(&free_b, &total_b));
  return std::min<size_t>(free_b / 2, (size_t)4 << 30);
}

static int ivf_grid(size_t work, int block) { return (int)std::min<size_t>((work + block - 1) / block, (size_t)ctx().num_cus * 16); }

static void ivf_pad(const void *src, size_t itemsize, size_t rows, int f, int f_pad, float *dst) {
  if (!rows) return;
  IMP_PROF("ivf_pad");
  const int grid = ivf_grid(rows * f_pad, 256);
  if (itemsize == 4) pad_rows(grid, static_cast<const float *>(src), dst, rows, f, f_pad);
  else pad_rows(grid, static_cast<const __half *>(src), dst, rows, f, f_pad);
  IMP_CHECK_HIP(hipGetLastError());
}

// scratch of one grouping of at most n_max elements by nkeys keys
struct IvfGrouper {
  int nkeys = 0, nruns = 0;
  int64_t n_max = 0;
  DeviceArray<unsigned> &cnt;  // the caller's, grown here
  DeviceArray<int32_t> totals;
  IvfGrouper(int64_t n_max_, int nkeys_, DeviceArray<unsigned> &cnt_) : nkeys(nkeys_), n_max(n_max_), cnt(cnt_) {
    nruns = (int)std::max<int64_t>(1, std::min<int64_t>((n_max + kIvfRun - 1) / kIvfRun, kIvfMaxCounters / nkeys));
    cnt.reserve((size_t)nruns * nkeys);
    totals.alloc(nkeys);
  }
  // off[nkeys + 1], order[n]: the elements by (key, element index); inv[n] (nullable): an element's place in `order`
  void run(const int32_t *keys, int64_t n, int32_t *off, int32_t *order, int32_t *inv) {
    IMP_PROF("ivf_group");
    const int64_t per = (n + nruns - 1) / nruns;
    const int run = (int)std::max<int64_t>(64, (per + 63) / 64 * 64);
    const int used = (int)std::max<int64_t>(1, (n + run - 1) / run);
    IMP_CHECK_HIP(hipMemsetAsync(cnt.data(), 0, (size_t)used * nkeys * sizeof(unsigned), stream()));
    if (n) hipLaunchKernelGGL(ivf_group_hist_kernel, dim3(used), dim3(64), 0, stream(), keys, n, run, nkeys, cnt.data());
    hipLaunchKernelGGL(ivf_group_colscan_kernel, dim3((nkeys + 255) / 256), dim3(256), 0, stream(), cnt.data(), used, nkeys, totals.data());
    hipLaunchKernelGGL(ivf_exclusive_scan_kernel, dim3(1), dim3(1024), 0, stream(), totals.data(), nkeys, off);
    if (n) hipLaunchKernelGGL(ivf_group_scatter_kernel, dim3(used), dim3(64), 0, stream(), keys, n, run, nkeys, cnt.data(), off, order, inv);
    IMP_CHECK_HIP(hipGetLastError());
  }
};

// the plans and the launch of one grouped (or dense) product
struct IvfProduct {
  DeviceArray<int32_t> dense_off;  // list_off[2], pair_off[2] of a dense product
  DeviceArray<int32_t> tile_off;   // nlist + 1
  DeviceArray<int64_t> score_base; // nlist + 1
  explicit IvfProduct(int nlist) {
    dense_off.alloc(4);
    tile_off.alloc((size_t)nlist + 1);
    score_base.alloc((size_t)nlist + 1);
  }
  void launch(const IvfScanArgs &a) {
    hipLaunchKernelGGL(ivf_plan_kernel, dim3(1), dim3(1024), 0, stream(), a.list_off, a.pair_off, a.nlist, tile_off.data(), score_base.data());
    hipLaunchKernelGGL(ivf_scan_kernel, dim3(ctx().num_cus * 8), dim3(256), 0, stream(), a);
    IMP_CHECK_HIP(hipGetLastError());
  }
  // S[rows x cols] = Q[rows x f_pad] . V[cols x f_pad]^T
  void dense(const float *Q, int rows, const float *V, int cols, int f_pad, float *S) {
    IMP_PROF("ivf_dense_scores");
    hipLaunchKernelGGL(ivf_dense_plan_kernel, dim3(1), dim3(1), 0, stream(), rows, cols, dense_off.data(), dense_off.data() + 2);
    launch(IvfScanArgs{Q, V, S, dense_off.data(), dense_off.data() + 2, nullptr, tile_off.data(), score_base.data(), 1, 1, f_pad});
  }
};

}  // namespace imp

using namespace imp;

extern "C" int imp_ivf_build(const imp_matrix *vectors, int nlist, int iterations, const int32_t *init_rows, imp_ivf **out) {
  return guarded([&] {
    if (!vectors || !init_rows || !out) throw std::invalid_argument("ivf_build: NULL argument");
    if (vectors->itemsize != 4 && vectors->itemsize != 2) throw std::invalid_argument("ivf_build: vectors must be fp32 or fp16");
    const size_t n = vectors->rows, f = vectors->cols;
    if (n < 1 || n > (size_t)INT32_MAX) throw std::invalid_argument("ivf_build: the row count must lie in 1 .. 2^31 - 1");
    if (f < 1 || f > 1024) throw std::invalid_argument("ivf_build: the column count must lie in 1 .. 1024");
    if (nlist < 1 || (size_t)nlist > n) throw std::invalid_argument("ivf_build: nlist must lie in 1 .. rows");
    if (iterations < 0) throw std::invalid_argument("ivf_build: iterations must be >= 0");
    for (int c = 0; c < nlist; ++c)
      if (init_rows[c] < 0 || (size_t)init_rows[c] >= n) throw out_of_range_error("ivf_build: initial row id outside the matrix");
    auto ix = std::make_unique<imp_ivf>();
    ix->n = n, ix->f = f, ix->f_pad = (int)((f + 3) / 4 * 4), ix->nlist = nlist;
    ix->budget = ivf_default_budget();
    const int f_pad = ix->f_pad;

    DeviceArray<float> vec;
    vec.alloc(n * f_pad);
    ivf_pad(vectors->as(), vectors->itemsize, n, (int)f, f_pad, vec.data());
    DeviceArray<int32_t> init;
    init.upload(init_rows, nlist);
    ix->centroids.alloc((size_t)nlist * f_pad);
    hipLaunchKernelGGL(ivf_init_centroids_kernel, dim3(nlist), dim3(256), 0, stream(), vec.data(), init.data(), f_pad, ix->centroids.data());
    IMP_CHECK_HIP(hipGetLastError());

    // assignment scores in chunks of rows that fit the budget
    const size_t chunk = std::min<size_t>(n, std::max<size_t>(kIvfBM, ix->budget / (sizeof(float) * nlist)));
    DeviceArray<float> S;
    S.alloc(chunk * nlist);
    DeviceArray<int32_t> assign;
    assign.alloc(n);
    ix->list_off.alloc((size_t)nlist + 1);
    ix->list_ids.alloc(n);
    IvfProduct product(1);
    DeviceArray<unsigned> group_cnt;
    IvfGrouper grouper((int64_t)n, nlist, group_cnt);
    for (int it = 0; it <= iterations; ++it) {
      for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t rows = std::min(chunk, n - r0);
        product.dense(vec.data() + r0 * f_pad, (int)rows, ix->centroids.data(), nlist, f_pad, S.data());
        IMP_PROF("ivf_argmax");
        hipLaunchKernelGGL(ivf_argmax_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream(), S.data(), (int64_t)rows, nlist,
                           assign.data() + r0);
        IMP_CHECK_HIP(hipGetLastError());
      }
      grouper.run(assign.data(), (int64_t)n, ix->list_off.data(), ix->list_ids.data(), nullptr);
      if (it == iterations) break;  // the lists now stand against the final centroids
      IMP_PROF("ivf_update_centroids");
      hipLaunchKernelGGL(ivf_update_centroids_kernel, dim3(nlist), dim3(256), 0, stream(), vec.data(), ix->list_off.data(),
                         ix->list_ids.data(), f_pad, ix->centroids.data());
      IMP_CHECK_HIP(hipGetLastError());
    }
    ix->list_vecs.alloc(n * f_pad);
    {
      IMP_PROF("ivf_gather_rows");
      hipLaunchKernelGGL(ivf_gather_rows_kernel, dim3(ivf_grid(n * (f_pad / 4), 256)), dim3(256), 0, stream(), vec.data(),
                         ix->list_ids.data(), n, f_pad, ix->list_vecs.data());
      IMP_CHECK_HIP(hipGetLastError());
    }
    std::vector<int32_t> off((size_t)nlist + 1);
    IMP_CHECK_HIP(hipMemcpyAsync(off.data(), ix->list_off.data(), off.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream()));
    sync();
    std::vector<int64_t> lens(nlist);
    for (int l = 0; l < nlist; ++l) lens[l] = off[l + 1] - off[l];
    std::sort(lens.begin(), lens.end(), std::greater<int64_t>());
    ix->lens_desc_sum.assign((size_t)nlist + 1, 0);
    for (int l = 0; l < nlist; ++l) ix->lens_desc_sum[l + 1] = ix->lens_desc_sum[l] + lens[l];
    *out = ix.release();
  });
}

extern "C" int imp_ivf_shape(const imp_ivf *ix, size_t *rows, size_t *cols, int *nlist) {
  return guarded([&] {
    if (!ix) throw std::invalid_argument("ivf_shape: NULL argument");
    if (rows) *rows = ix->n;
    if (cols) *cols = ix->f;
    if (nlist) *nlist = ix->nlist;
  });
}

extern "C" int imp_ivf_set_temp_memory(imp_ivf *ix, size_t max_temp_memory) {
  return guarded([&] {
    if (!ix) throw std::invalid_argument("ivf_set_temp_memory: NULL argument");
    sync();
    ix->ws = imp_ivf::Workspace();
    ix->budget = max_temp_memory ? max_temp_memory : ivf_default_budget();
  });
}

extern "C" int imp_ivf_lists(const imp_ivf *ix, float *centroids, int64_t *list_offsets, int32_t *list_ids) {
  return guarded([&] {
    if (!ix) throw std::invalid_argument("ivf_lists: NULL argument");
    std::vector<int32_t> off((size_t)ix->nlist + 1);
    if (centroids)
      IMP_CHECK_HIP(hipMemcpy2DAsync(centroids, ix->f * sizeof(float), ix->centroids.data(), (size_t)ix->f_pad * sizeof(float),
                                     ix->f * sizeof(float), ix->nlist, hipMemcpyDeviceToHost, stream()));
    if (list_offsets)
      IMP_CHECK_HIP(hipMemcpyAsync(off.data(), ix->list_off.data(), off.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream()));
    if (list_ids)
      IMP_CHECK_HIP(hipMemcpyAsync(list_ids, ix->list_ids.data(), ix->n * sizeof(int32_t), hipMemcpyDeviceToHost, stream()));
    sync();
    if (list_offsets) std::copy(off.begin(), off.end(), list_offsets);
  });
}

extern "C" int imp_ivf_search(imp_ivf *ix, const imp_matrix *query, int k, int nprobe, int32_t *indices, float *distances,
                              int32_t *probes) {
  return guarded([&] {
    if (!ix || !query || !indices || !distances) throw std::invalid_argument("ivf_search: NULL argument");
    if (k < 1 || k > kIvfMaxK) throw std::invalid_argument("ivf_search: k must lie in 1 .. 1024");
    if (nprobe < 1) throw std::invalid_argument("ivf_search: nprobe must be >= 1");
    if (query->itemsize != 4 && query->itemsize != 2) throw std::invalid_argument("ivf_search: queries must be fp32 or fp16");
    if (query->cols != ix->f) throw std::invalid_argument("ivf_search: the queries' column count differs from the index's");
    const size_t nq = query->rows;
    const int nlist = ix->nlist, f_pad = ix->f_pad, P = std::min(nprobe, nlist);
    if (P > kIvfMaxK) throw std::invalid_argument("ivf_search: no more than 1024 lists can be probed");  // zero queries too
    if (!nq) return;
    int kpad = 1;
    while (kpad < k) kpad <<= 1;
    // a query's share of the temporaries, its scores at worst those of the P longest lists
    const size_t max_cand = (size_t)std::max<int64_t>(ix->lens_desc_sum[P], nlist);
    const size_t per_query = sizeof(float) * (max_cand + f_pad + P + k) + sizeof(int32_t) * (3 * (size_t)P + k);
    const size_t chunk = std::min<size_t>(nq, std::max<size_t>(1, ix->budget / per_query));
    if (chunk * P > (size_t)INT32_MAX) throw std::invalid_argument("ivf_search: too many (query, probe) pairs in one chunk");

    imp_ivf::Workspace &ws = ix->ws;
    DeviceArray<float> &Q = ws.Q, &S = ws.S, &probe_dist = ws.probe_dist, &out_dist = ws.out_dist;
    DeviceArray<int32_t> &d_probes = ws.probes, &sorted = ws.sorted, &inv = ws.inv, &pair_off = ws.pair_off, &out_ids = ws.out_ids;
    Q.reserve(chunk * f_pad), S.reserve(chunk * max_cand), probe_dist.reserve(chunk * P), out_dist.reserve(chunk * k);
    d_probes.reserve(chunk * P), sorted.reserve(chunk * P), inv.reserve(chunk * P), pair_off.reserve((size_t)nlist + 1);
    out_ids.reserve(chunk * k);
    IvfProduct coarse(1), scan(nlist);
    IvfGrouper grouper((int64_t)(chunk * P), nlist, ws.group_cnt);
    int ppad = 1;
    while (ppad < P) ppad <<= 1;

    for (size_t q0 = 0; q0 < nq; q0 += chunk) {
      const size_t rows = std::min(chunk, nq - q0);
      ivf_pad(query->as<char>() + q0 * ix->f * query->itemsize, query->itemsize, rows, (int)ix->f, f_pad, Q.data());
      coarse.dense(Q.data(), (int)rows, ix->centroids.data(), nlist, f_pad, S.data());
      {
        IMP_PROF("ivf_select_probes");
        const IvfSelectArgs a{S.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, nlist, P, ppad, d_probes.data(), probe_dist.data()};
        hipLaunchKernelGGL(ivf_select_kernel, dim3((unsigned)rows), dim3(256), 0, stream(), a);
        IMP_CHECK_HIP(hipGetLastError());
      }
      if (probes)
        IMP_CHECK_HIP(hipMemcpyAsync(probes + q0 * P, d_probes.data(), rows * P * sizeof(int32_t), hipMemcpyDefault, stream()));
      grouper.run(d_probes.data(), (int64_t)(rows * P), pair_off.data(), sorted.data(), inv.data());
      {
        IMP_PROF("ivf_scan");
        scan.launch(IvfScanArgs{Q.data(), ix->list_vecs.data(), S.data(), ix->list_off.data(), pair_off.data(), sorted.data(),
                                scan.tile_off.data(), scan.score_base.data(), nlist, P, f_pad});
      }
      {
        IMP_PROF("ivf_select");
        const IvfSelectArgs a{S.data(), d_probes.data(), inv.data(), pair_off.data(), ix->list_off.data(), ix->list_ids.data(),
                              scan.score_base.data(), P, 0, k, kpad, out_ids.data(), out_dist.data()};
        hipLaunchKernelGGL(ivf_select_kernel, dim3((unsigned)rows), dim3(256), 0, stream(), a);
        IMP_CHECK_HIP(hipGetLastError());
      }
      IMP_CHECK_HIP(hipMemcpyAsync(indices + q0 * k, out_ids.data(), rows * k * sizeof(int32_t), hipMemcpyDefault, stream()));
      IMP_CHECK_HIP(hipMemcpyAsync(distances + q0 * k, out_dist.data(), rows * k * sizeof(float), hipMemcpyDefault, stream()));
    }
    sync();
  });
}

extern "C" int imp_ivf_destroy(imp_ivf *ix) {
  return guarded([&] { delete ix; });
}
