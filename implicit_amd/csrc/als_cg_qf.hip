// K1f: the 32-entry fp32 tile of the team kernel (als_qf_common.h has the kernel and its design) with als_cg_qfteam_kernel --
// the mid rows of fp32 storage and the f = 64 short rows of both storages -- the f = 128 short-row kernel
// als_cg_qfgroup_kernel, and the two chained launches of fp32 storage at f = 128 (als_cg_qfteam_chain_kernel,
// als_cg_qfwide_chain_kernel).
//
// Arithmetic contract: the oracle's CG (implicit/cpu/_als.pyx:152-248).
#include <type_traits>

#include <algorithm>

#include "als_cg_fixup.h"
#include "als_nm_image.h"
#include "als_qf_common.h"
#include "common.h"

namespace imp {

// The fp32 tile: 32 entries per wavefront, 8 per 16-lane group; lane (g, m) keeps the F / 16 expanded slots of each of its
// entries as F / 32 packed pairs (64 registers at f = 128).  fp16 storage is converted at the load.
template <typename ST> struct Tile32 {
  typedef f32x2 elem;
  static constexpr int T = 32;
  static constexpr bool ROLL = std::is_same<ST, float>::value;  // fp16 storage converts at the load: no rolling gather
  // entry t of the slice in lanes t and t + 32
  static __device__ __forceinline__ void fetch(const int32_t *indices, const float *data, int lane, int k0, int end, int &col, float &c) {
    fetch_entries(indices, data, lane, k0, end, col, c);
  }
  template <int H> static __device__ __forceinline__ void gather(elem (&yq)[H], const ST *p) {
#pragma unroll
    for (int h = 0; h < H; h += 2) {  // expanded slots 2 h .. 2 h + 3 = 4 consecutive factors
      const float4 v = load4(p + 32 * h);
      yq[h] = f32x2{v.x, v.y}, yq[h + 1] = f32x2{v.z, v.w};
    }
  }
  template <int H> static __device__ __forceinline__ float dot(const elem (&yq)[H], const f32x2 (&ve)[H]) {
    f32x2 s = yq[0] * ve[0];
#pragma unroll
    for (int h = 1; h < H; ++h) s = __builtin_elementwise_fma(yq[h], ve[h], s);
    return s.x + s.y;
  }
  template <int H> static __device__ __forceinline__ void axpy(const elem (&yq)[H], float w, f32x2 (&ae)[H]) {
    const f32x2 w2 = {w, w};
#pragma unroll
    for (int h = 0; h < H; ++h) ae[h] = __builtin_elementwise_fma(w2, yq[h], ae[h]);
  }
};

template <int F, int WPR, int BLOCK, typename ST>
__global__ __launch_bounds__(BLOCK, F == 64 ? 8 : 4) void als_cg_qfteam_kernel(const int32_t *__restrict__ order, int first, int count,
                                                                 const int32_t *__restrict__ indptr,
                                                                 const int32_t *__restrict__ indices,
                                                                 const float *__restrict__ data, ST *__restrict__ X,
                                                                 const ST *__restrict__ Y, const float *__restrict__ A0,
                                                                 int cg_steps) {
  team_rows<Tile32<ST>, F, WPR, BLOCK>(order, first, count, indptr, indices, data, X, Y, A0, cg_steps);
}

template <int F, int WPR, int BLOCK, typename T>
static void launch_qfteam(const imp_csr *C, int first, int count, T *X, const T *Y, const float *A0, int cg_steps,
                          const char *name) {
  if (count <= 0) return;
  constexpr int WAVES = BLOCK / 64, TEAMS = WAVES / WPR;
  size_t lds = team_lds_bytes<F, WPR, BLOCK, Tile32<T>::T>();
  auto kern = als_cg_qfteam_kernel<F, WPR, BLOCK, T>;
  allow_dynamic_lds(kern, lds);
  int per_cu = (int)std::max<size_t>(1, std::min<size_t>(2048 / BLOCK, (160 * 1024) / lds));
  // als_cg_q.hip launch_qteam; the 16-wave team at f = 64 (16 KB of gramian to stage, two workgroups per CU) takes 2 as well:
  // configs[1]-shaped CG 1.47 -> 1.42 ms, and a fixed share on a contended CU is what took seconds once (HISTORY.md section 6)
  constexpr int kBaseOversub = WPR <= 4 ? 4 : (WPR == 8 ? 2 : (F == 64 ? 2 : 1));
  int grid = std::min((count + TEAMS - 1) / TEAMS, ctx().num_cus * per_cu * std::max(kBaseOversub, ctx().oversub));
  IMP_PROF(name);
  kern<<<grid, BLOCK, lds, stream()>>>(C->order.data(), first, count, C->indptr.data(), C->indices.data(), C->data.data(), X, Y,
                                      A0, cg_steps);
  IMP_CHECK_HIP(hipGetLastError());
}

// ---- the three 512-thread classes in one persistent launch ---------------------------------------------------------------
// (128,256], (64,128] and (32,64] -- team widths 8, 4, 2 -- have the same workgroup shape and nearly the same LDS and register
// needs.  As three launches each of them ends in a tail in which the device drains, and starts with a ramp in which every
// workgroup stages the gramian again -- up to four times per slot inside a launch, which oversubscribed its grid to even its
// fixed shares out.  Here the grid is exactly the resident workgroups; a workgroup stages the gramian once and runs the
// classes in order, and inside a class its teams draw their rows by ticket (team_rows, TICKETS): the schedule is
// longest-first, so tickets balance a class dynamically, and a workgroup that runs out of one class starts the next at
// once.  No workgroup waits for another; the counters of the classes' queues are the only global state, and they are never
// reset (team_tickets.h).  Every row's arithmetic is that of its class kernel, and no row depends on which team solves it, or when.
//
// At its head the launch carries the FINISH ITEMS of the long-row path (nm_finish_items, als_nm_image.h; long_tail_route.h says
// when): the normal-matrix kernel has ended behind a kernel boundary, workgroup b sums the partial images of the rows b,
// b + grid, ... into the LDS this launch holds anyway and runs their CG there, wavefronts 4 - 7 idle at the barriers.  A few
// hundred items of 10 - 100 us ahead of ticketed classes of a millisecond: the tickets absorb them.
struct ChainClassArgs {
  int first[ChainTickets::kClasses], count[ChainTickets::kClasses];
  unsigned base[ChainTickets::kClasses][ChainTickets::kQueues];
};
static_assert(ChainTickets::kQueues == kTicketQueues, "queues of a ticketed class");
template <int F> constexpr size_t chain_lds_bytes() {
  return std::max(team_lds_bytes<F, 8, 512, 32>(), std::max(team_lds_bytes<F, 4, 512, 32>(), team_lds_bytes<F, 2, 512, 32>()));
}
template <int F, typename ST>
__global__ __launch_bounds__(512, F == 64 ? 8 : 4) void als_cg_qfteam_chain_kernel(const int32_t *__restrict__ order, ChainClassArgs cls,
                                                                                  unsigned *__restrict__ counters,
                                                                                  const int32_t *__restrict__ indptr,
                                                                                  const int32_t *__restrict__ indices,
                                                                                  const float *__restrict__ data, ST *__restrict__ X,
                                                                                  const ST *__restrict__ Y, const float *__restrict__ A0,
                                                                                  int cg_steps, NmFinishArgs finish) {
  static_assert(Tile32<ST>::T == 32, "chain_lds_bytes");
  static_assert(NmLayout<F>::lds_floats * sizeof(float) <= chain_lds_bytes<F>(), "the finish items work in the chain's own LDS");
  if (finish.n_multi > 0) {  // uniform over the grid
    extern __shared__ __attribute__((aligned(16))) float smem[];
    nm_finish_items<F, ST, 512>(finish, X, cg_steps, smem);  // returns behind a barrier: the gramian may overwrite the image
  }
  team_stage_gramian<F, 512>(A0);
  bool entered = false;  // a class has run: its LDS layout is live until every wavefront of the workgroup has left it
  static_for<ChainTickets::kClasses>([&](auto Cc) {
    constexpr int C = decltype(Cc)::value, WPR = 8 >> C;
    if (cls.count[C] > 0) {  // uniform over the grid
      if (entered) __syncthreads();
      entered = true;
      team_rows<Tile32<ST>, F, WPR, 512, true, false>(order, cls.first[C], cls.count[C], indptr, indices, data, X, Y, A0, cg_steps,
                                                      counters + (C * kTicketQueues + blockIdx.x % kTicketQueues) * ChainTickets::kCounterStride,
                                                      cls.base[C][blockIdx.x % kTicketQueues]);
    }
  });
}

// workgroups per CU of a 512-thread team kernel with `lds` bytes of LDS (launch_qfteam)
static int team512_per_cu(size_t lds) { return (int)std::max<size_t>(1, std::min<size_t>(2048 / 512, (160 * 1024) / lds)); }

template <typename T>
void launch_team_chain(const imp_csr *C, int f, const int (&first)[3], const int (&count)[3], T *X, const T *Y, const float *A0, int cg_steps,
                       const char *name, const NmTail *finish) {
  if constexpr (std::is_same<T, float>::value) {
    auto run = [&](auto Fc) {
      constexpr int F = decltype(Fc)::value;
      if (count[0] <= 0 && count[1] <= 0 && count[2] <= 0) {
        if (finish) throw std::logic_error("launch_team_chain: finish items without a launch to carry them");
        return;
      }
      NmFinishArgs fin;
      if (finish)
        fin = NmFinishArgs{finish->n_multi, finish->plan.rows, finish->plan.row_seg, finish->gram_img, finish->partial, finish->ctl, finish->fix_rows};
      const size_t lds = chain_lds_bytes<F>();
      auto kern = als_cg_qfteam_chain_kernel<F, T>;
      allow_dynamic_lds(kern, lds);
      // exactly the resident workgroups: tickets do what oversubscription did (and every queue needs a workgroup)
      const int grid = std::max(ctx().num_cus * team512_per_cu(lds), ChainTickets::kQueues);
      ChainClassArgs cls;
      const int teams[3] = {1, 2, 4};  // per workgroup of 8 wavefronts
      for (int c = 0; c < 3; ++c) {
        if (count[c] >= ChainTickets::kMaxCount) throw std::invalid_argument("launch_team_chain: too many rows in a class");
        cls.first[c] = first[c], cls.count[c] = std::max(count[c], 0);
      }
      Context &cx = ctx();
      // zeroed once, on the library stream
      cx.chain_counters.reserve((size_t)ChainTickets::kClasses * ChainTickets::kQueues * ChainTickets::kCounterStride, true);
      ChainTickets after = cx.chain_tickets;
      after.launch(cls.count, grid, teams, cls.base);
      IMP_PROF(name);
      kern<<<grid, 512, lds, stream()>>>(C->order.data(), cls, cx.chain_counters.data(), C->indptr.data(), C->indices.data(),
                                        C->data.data(), X, Y, A0, cg_steps, fin);
      IMP_CHECK_HIP(hipGetLastError());
      cx.chain_tickets = after;  // a launch that was not queued draws nothing
    };
    // f = 64 keeps its per-class launches: its team kernels sit exactly at the 64 registers of 8 waves per SIMD, and the three
    // row loops in one kernel do not fit (the chain compiles to 32 bytes of scratch per lane there; none at f = 128: 127 VGPRs)
    if (f == 128) run(idx_t<128>{});
    else throw std::invalid_argument("launch_team_chain: f must be 128");
  } else {
    throw std::invalid_argument("launch_team_chain: fp32 storage only (float16 storage runs its classes on the packed tiles)");
  }
}
template void launch_team_chain<float>(const imp_csr *, int, const int (&)[3], const int (&)[3], float *, const float *, const float *, int,
                                       const char *, const NmTail *);
template void launch_team_chain<__half>(const imp_csr *, int, const int (&)[3], const int (&)[3], __half *, const __half *, const float *,
                                        int, const char *, const NmTail *);

// ---- short rows (<= 32 nnz) at f = 128: one wave per row, 16 rows per workgroup in lock step --------------------------------
// The waves publish their operands in LDS; the dense part of a pass is ONE product A0 . P^T for the 16 rows, its 16-factor output
// tiles x K-slices dealt to the 16 waves, the results back through LDS.  Round 3 on top of it:
//   * the operand a wave has just published is read back EXPANDED (two ds_read_b128) instead of 6 permlane swaps;
//   * weight table, pair-wise DPP reduction, v_rcp divisions, last step on the scalar p . A p as in the team kernel;
//   * rolling gather: a workgroup holds its CU alone (its LDS), so while its 16 waves waited for the gathers of a new group of
//     rows the CU did nothing; the last pass of a group now re-fills each pair of tile registers with the next group's entries
//     as soon as the pair is done;
//   * the product on the bf16 matrix cores with three-term operands, and the waves staggered over the two pipes (below).  The
//     exact-fp32 MFMA product and the unstaggered order (IMP_SHORT_BF16X3 / IMP_SHORT_STAGGER until round 5) are gone;
//     HISTORY.md section 4.1 has their measurements.
typedef float f32x4 __attribute__((ext_vector_type(4)));
template <int F> struct QFGroupCfg {
  static constexpr int LD = F + 8;          // P / Out row stride in LDS, floats (conflict-free b128 fragment reads)
  static constexpr int LDB = F + 8;         // row stride of the bf16 terms
  static constexpr int NT = F / 16;         // 16-factor output tiles
  static constexpr int KH = 16 / NT;        // K-slices so that NT * KH == 16 waves
  static constexpr int KB = (F / 16) / KH;  // 16-factor k-blocks per wave
  // the gramian and the operands as three bf16 terms each (hi + mid + lo = the fp32 value to 2^-24), then the fp32 operands,
  // the K-slice partial products and the weight tables; the fp32 gramian image is not kept
  static constexpr size_t lds_bytes = (size_t)3 * F * LDB * 2 + (size_t)3 * 16 * LDB * 2 +
                                      ((size_t)16 * LD + (size_t)KH * 16 * LD + 16 * 64) * sizeof(float);
};
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
// x = hi + mid + lo + O(2^-24 |x|): every term the nearest bf16 of what is left (the subtractions are exact in fp32)
__device__ __forceinline__ void split_bf16(float x, __bf16 &hi, __bf16 &mid, __bf16 &lo) {
  hi = (__bf16)x;
  const float r1 = x - (float)hi;
  mid = (__bf16)r1;
  lo = (__bf16)(r1 - (float)mid);
}

// tile part of a pass: acc (compact) = sum over the resident entries of w y, operand read expanded from `vrow` (natural order)
//   FIRST: w = c+ - (|c|-1) y.x   else: w = (|c|-1) y.v
//   LAST : the last CG step needs p . A p only (fused_pass): no weights, no axpys, acc is left alone; RETURNS this lane's share
//          of sum (|c|-1) (y . p)^2 -- the sum of the shares over the wave is the tile part of p . A p
//   ROLL : pair P of the tile is re-filled with the next group's entries once it is done (with LAST only)
template <int F, bool FIRST, bool LAST, bool ROLL, typename ST>
__device__ __forceinline__ float tile_pass(f32x2 (&y)[8][F / 32], float *cw, int cnt, const float *vrow, float (&acc)[F / 64], int lane,
                                          int cnt_nx, int &col_nx, float &c_nx, const ST *__restrict__ Y) {
  using Tile = Tile32<ST>;
  constexpr int FE = F / 16, H = FE / 2;
  static_assert(!(FIRST && LAST) && (LAST || !ROLL), "pass form");
  if constexpr (ROLL) {  // one wait for the staged entries, before any rolling gather (fused_pass)
    col_nx = opaque(col_nx);
    c_nx = __int_as_float(opaque(__float_as_int(c_nx)));
  }
  f32x2 ve[H], ae[H];
  const float *cwg;
  {
    const int ln = opaque(lane);
    const int g = ln >> 4, m = ln & 15;
#pragma unroll
    for (int e = 0; e < FE; e += 4) {
      const float4 t = *reinterpret_cast<const float4 *>(vrow + 16 * e + 4 * m);
      ve[e / 2] = f32x2{t.x, t.y}, ve[e / 2 + 1] = f32x2{t.z, t.w};
    }
    cwg = cw + g;
    if constexpr (LAST) cwg += 4 * (m >> 3);  // the weight of the total this lane holds after reduce_pair
  }
#pragma unroll
  for (int h = 0; h < H; ++h) ae[h] = f32x2{0.f, 0.f};
  float s8 = 0.f;  // LAST: every entry is counted in 8 lanes
  auto partial = [&](int q) { return Tile::template dot<H>(y[q], ve); };
  auto axpy = [&](int q, float w) { Tile::template axpy<H>(y[q], w, ae); };
  static_for<4>([&](auto Pc) {
    constexpr int P = decltype(Pc)::value;
    if (8 * P < cnt) {  // wave-uniform
      const float cm1_0 = cwg[8 * P];
      float cm1_1 = 0.f, cp_0 = 0.f, cp_1 = 0.f;
      if constexpr (!LAST) cm1_1 = cwg[8 * P + 4];
      if constexpr (FIRST) cp_0 = cwg[32 + 8 * P], cp_1 = cwg[32 + 8 * P + 4];
      const float u = reduce_pair(partial(2 * P), partial(2 * P + 1));
      if constexpr (LAST) {
        s8 = fmaf(cm1_0 * u, u, s8);
      } else {
        const float w0 = FIRST ? fmaf(-cm1_0, row_bcast_from<0>(u), cp_0) : cm1_0 * row_bcast_from<0>(u);
        const float w1 = FIRST ? fmaf(-cm1_1, row_bcast_from<8>(u), cp_1) : cm1_1 * row_bcast_from<8>(u);
        axpy(2 * P, w0);
        axpy(2 * P + 1, w1);
      }
    }
    if constexpr (ROLL) {
      if (8 * P < cnt_nx) gather_pair<Tile, F, P>(y, cw, col_nx, c_nx, cnt_nx, Y, lane);
    }
  });
  if constexpr (LAST) {
    return 0.125f * s8;
  } else {
    float aes[FE];
#pragma unroll
    for (int h = 0; h < H; ++h) aes[2 * h] = ae[h].x, aes[2 * h + 1] = ae[h].y;
    reduce_expanded<F>(aes, acc);
    return 0.f;
  }
}

// The short-row kernel has two parts, like a team kernel (als_qf_common.h): a workgroup prologue -- the gramian as three bf16
// planes into LDS -- and the group loop.  The per-class kernel runs them in sequence; the chain of the two 1024-thread classes
// (als_cg_qfwide_chain_kernel) runs them after the team-16 class, over the same allocation.
template <int F> __device__ __forceinline__ void group_stage_gramian(const float *__restrict__ A0) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int LDB = QFGroupCfg<F>::LDB;
  __bf16 *A0b = reinterpret_cast<__bf16 *>(smem);
  for (int e = threadIdx.x; e < F * F; e += 1024) {
    int r = e / F, c = e - r * F;
    __bf16 h, m, l;
    split_bf16(A0[e], h, m, l);
    A0b[r * LDB + c] = h, A0b[(size_t)F * LDB + r * LDB + c] = m, A0b[(size_t)2 * F * LDB + r * LDB + c] = l;
  }
  __syncthreads();
}

// The group loop: rows [first, first + count) of the schedule in groups of 16 consecutive rows, one wavefront per row.
//   TICKETS false: a workgroup's groups are blockIdx.x + k gridDim.x -- the per-class kernel.
//   TICKETS true : a workgroup draws its groups by ticket, by the protocol of team_rows (team_tickets.h) with the workgroup as
//     the team and the group as the row: group k belongs to queue k mod 8, workgroup b serves queue b mod 8; with N workgroups
//     on a queue, workgroup g starts with the tickets g, g + N, g + 2 N, g + 3 N -- the four groups the metadata pipeline holds
//     -- and every later one is an atomic increment of *counter.  Lane 0 of wave 0 draws after the first operand of a group
//     is published, takes the value at the end of that pass and leaves the ticket (clamped to the queue's end) in one LDS
//     word before the barrier that ends the pass; all 16 waves read it after that barrier.  The pass chain gains no barrier,
//     wait or poll.  A workgroup whose newest ticket is at or past the queue's end draws no more.
template <int F, typename ST, bool TICKETS = false>
__device__ __forceinline__ void group_rows(const int32_t *__restrict__ order, int first, int count, const int32_t *__restrict__ indptr,
                                           const int32_t *__restrict__ indices, const float *__restrict__ data, ST *__restrict__ X,
                                           const ST *__restrict__ Y, int cg_steps, unsigned *counter = nullptr, unsigned base = 0u) {
  using Cfg = QFGroupCfg<F>;
  constexpr int FC = F / 64, FE = F / 16, LD = Cfg::LD;
  constexpr bool ROLL = Tile32<ST>::ROLL;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int LDB = Cfg::LDB;
  // [A0 hi | mid | lo, bf16 F x LDB each][Pb hi | mid | lo, 16 x LDB][Ps][Outs][cws]([ticket word], TICKETS)
  __bf16 *A0b = reinterpret_cast<__bf16 *>(smem);       // term t at A0b + t F LDB
  __bf16 *Pb = A0b + (size_t)3 * F * LDB;               // term t at Pb + t 16 LDB
  float *Ps = reinterpret_cast<float *>(Pb + (size_t)3 * 16 * LDB);  // [16][LD] operands (natural order)
  float *Outs = Ps + 16 * LD;                          // [KH][16][LD]  K-slice partial products
  float *cws = Outs + (size_t)Cfg::KH * 16 * LD;       // [16][64]  per-entry weights (gather_pair)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float *prow = Ps + (size_t)wave * LD;
  float *cw = cws + (size_t)wave * 64;
  const unsigned cf = (unsigned)QL<F>::cfactor(lane, 0);  // this lane's compact slots inside a natural-order vector

  // this wave's operand for the 16-row product, in natural order and as three bf16 terms; every wave of the workgroup takes the
  // barrier (inactive rows publish 0)
  auto publish = [&](const float (&vec)[FC], bool valid) {
    if constexpr (FC == 2) *reinterpret_cast<float2 *>(prow + cf) = valid ? make_float2(vec[0], vec[1]) : make_float2(0.f, 0.f);
    else prow[cf] = valid ? vec[0] : 0.f;
    bf16x2 t[3];  // (FC == 2: one packed pair per term)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      __bf16 h, m, l;
      split_bf16(valid ? vec[c] : 0.f, h, m, l);
      t[0][c] = h, t[1][c] = m, t[2][c] = l;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) *reinterpret_cast<bf16x2 *>(Pb + (size_t)k * 16 * LDB + (size_t)wave * LDB + cf) = t[k];
    __syncthreads();
  };
  auto product = [&]() {  // this wave's (output tile, K-slice) of A0 . P^T for the 16 rows -> Outs
    const int ti = wave % Cfg::NT, kh = wave / Cfg::NT;
    const int ln = opaque(lane);
    const int i = ln & 15, kq = ln >> 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    // fp32-equivalent product on the bf16 matrix cores: A0 = Ah + Am + Al, p = ph + pm + pl (each to 2^-24), and the six
    // partial products down to 2^-16 relative weight, smallest first, accumulated in fp32 -- 12 MFMAs of K = 32 per wave
    // and pass instead of 16 fp32 MFMAs of K = 4, at a quarter of the instruction time each, and on hardware the vector
    // pipe does not share (v_mfma_f32_16x16x4_f32 runs at the VECTOR rate and, measured, does not overlap with the tile
    // entries' packed FMAs; these do).  A and B fragments use the same (lane group, element) -> k assignment, which is all
    // the contraction needs.
    static_assert(Cfg::KB * 16 == 64, "three-term product: 64 k per wave");
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int k0 = kh * 64 + 32 * b + 8 * kq;
      const __bf16 *ar = A0b + (size_t)(16 * ti + i) * LDB + k0, *pr = Pb + (size_t)i * LDB + k0;
      const bf16x8 ah = *reinterpret_cast<const bf16x8 *>(ar), am = *reinterpret_cast<const bf16x8 *>(ar + (size_t)F * LDB),
                   al = *reinterpret_cast<const bf16x8 *>(ar + (size_t)2 * F * LDB);
      const bf16x8 ph = *reinterpret_cast<const bf16x8 *>(pr), pm = *reinterpret_cast<const bf16x8 *>(pr + (size_t)16 * LDB),
                   pl = *reinterpret_cast<const bf16x8 *>(pr + (size_t)2 * 16 * LDB);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, ph, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, pl, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, pm, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, ph, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, pm, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, ph, acc, 0, 0, 0);
    }
    *reinterpret_cast<float4 *>(Outs + (kh * 16 + i) * LD + 16 * ti + 4 * kq) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  };
  auto collect = [&](float (&out)[FC]) {  // after the barrier that follows the product: the K-slices of this wave's row
#pragma unroll
    for (int c = 0; c < FC; ++c) out[c] = 0.f;
#pragma unroll
    for (int h = 0; h < Cfg::KH; ++h) {
      const float *o = Outs + (h * 16 + wave) * LD + cf;
      if constexpr (FC == 2) {
        const float2 t = *reinterpret_cast<const float2 *>(o);
        out[0] += t.x, out[1] += t.y;
      } else {
        out[0] += o[0];
      }
    }
  };
  // Stagger: between the two barriers of a pass every wave has a matrix-pipe block (its 4 KB MFMAs of the 16-row product) and a
  // vector-pipe block (its own row's tile entries, which need only the operand it published itself).  With all waves of a
  // SIMD in the same block one pipe idled while the other worked (knock-outs: the product, the tile entries and the barriers
  // each "cost" 40 % of the kernel).  Waves 0-3 and 8-11 run the product first, waves 4-7 and 12-15 their tile entries
  // first -- two of each kind per SIMD (wave w sits on SIMD w mod 4) -- so the pipes work side by side, with the same
  // barriers and the same arithmetic.
  const bool product_first = ((wave >> 2) & 1) == 0;

  // A workgroup's groups are numbered g: the groups blockIdx.x + k gridDim.x themselves, or (TICKETS) the tickets of its queue,
  // ticket g being group 8 g + queue.  `groups` is the end of that numbering.
  const int queue = TICKETS ? (int)(blockIdx.x % kTicketQueues) : 0;
  const int all_groups = (count + 15) / 16;
  const int groups = TICKETS ? (all_groups - queue + kTicketQueues - 1) / kTicketQueues : all_groups;
  const int g_step = TICKETS ? (int)((gridDim.x - queue + kTicketQueues - 1) / kTicketQueues) : (int)gridDim.x;
  const int g_first = TICKETS ? (int)(blockIdx.x / kTicketQueues) : (int)blockIdx.x;
  // row of this wave in group g (groups past the end and rows past the count re-read the last row and stay invalid)
  auto row_of = [&](int g) { return (TICKETS ? kTicketQueues * g + queue : g) * 16 + wave; };
  auto row_id = [&](int g) { return order[first + min(row_of(g), count - 1)]; };  // uniform address: scalar load
  auto row_valid = [&](int g) { return g < groups && row_of(g) < count; };
  // TICKETS: the tickets of the three groups after the one at the top of the body, and the counter value of a draw on its way
  int t1 = g_first + g_step, t2 = g_first + 2 * g_step, t3 = g_first + 3 * g_step;
  unsigned drawn = 0u;
  unsigned *ticket_word = reinterpret_cast<unsigned *>(cws + 16 * 64);
  auto draw = [&]() {  // team_rows::draw
    if (lane == 0) asm volatile("global_atomic_add %0, %1, %2, off sc0" : "=v"(drawn) : "v"(counter), "v"(1u) : "memory");
  };
  auto take_draw = [&]() {  // wave 0, before the barrier that ends the group's first pass
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(drawn)::"memory");
    const unsigned t = min((unsigned)__builtin_amdgcn_readfirstlane(drawn) - base + 4u * (unsigned)g_step, (unsigned)groups);
    if (lane == 0) *ticket_word = t;
  };
  int id0 = row_id(g_first), id1 = row_id(t1), id2 = row_id(t2), id3 = row_id(t3);
  int b0 = indptr[id0], e0 = indptr[id0 + 1], b1 = indptr[id1], e1 = indptr[id1 + 1], b2 = indptr[id2], e2 = indptr[id2 + 1];
  int ent_col, ent_cnt = row_valid(g_first) ? e0 - b0 : 0;
  float ent_c;
  fetch_entries(indices, data, opaque(lane), b0, max(e0, b0 + 1), ent_col, ent_c);
  bool tile_ready = false;
  int cnt = 0;
  f32x2 y[8][FE / 2];
  float x[FC];
  auto kill = [](float (&v)[FC]) {
#pragma unroll
    for (int cc = 0; cc < FC; ++cc) v[cc] = 0.f;
  };
  kill(x);
  for (int g = g_first; g < groups;) {
    const bool valid = row_valid(g);
    int t_new = t3 + g_step;  // TICKETS: the ticket drawn during this group, or the queue's end
    ST *xrow = X + (size_t)id0 * F;
    if (!tile_ready) {  // first group, or this wave's previous row ended before its last pass
      cnt = ent_cnt;
      ent_col = opaque(ent_col);
      ent_c = __int_as_float(opaque(__float_as_int(ent_c)));
      static_for<4>([&](auto Pc) {
        constexpr int P = decltype(Pc)::value;
        if (8 * P < cnt) gather_pair<Tile32<ST>, F, P>(y, cw, ent_col, ent_c, cnt, Y, lane);
      });
      ent_cnt = row_valid(t1) ? e1 - b1 : 0;
      fetch_entries(indices, data, opaque(lane), b1, max(e1, b1 + 1), ent_col, ent_c);
      load_compact<F>(xrow, opaque(lane), x);
    }
    // ent_* now describe this wave's row of the next group (t1)
    float xc[FC], r[FC], p[FC], Ap[FC], sp[FC];
#pragma unroll
    for (int cc = 0; cc < FC; ++cc) xc[cc] = x[cc];
    // r = -(A0 x) + sum_k (c+ - (|c|-1) y.x) y        (_als.pyx:187-201)
    publish(xc, valid);
    const bool drawing = TICKETS && t3 < groups;  // uniform over the workgroup
    if constexpr (TICKETS) {
      // nothing else of wave 0 is in flight here: the iterate it has just published was its newest load
      if (drawing && wave == 0) draw();
    }
    if (!product_first) tile_pass<F, true, false, false, ST>(y, cw, cnt, prow, sp, lane, 0, ent_col, ent_c, Y);
    product();
    if (product_first) tile_pass<F, true, false, false, ST>(y, cw, cnt, prow, sp, lane, 0, ent_col, ent_c, Y);
    if constexpr (TICKETS) {
      if (drawing && wave == 0) take_draw();
    }
    __syncthreads();
    if constexpr (TICKETS) {
      // the word is written again only after the next group's first barrier, which every wave reaches after this read
      t_new = drawing ? (int)__builtin_amdgcn_readfirstlane(*reinterpret_cast<volatile unsigned *>(ticket_word)) : groups;
    }
    collect(Ap);
#pragma unroll
    for (int cc = 0; cc < FC; ++cc) p[cc] = r[cc] = sp[cc] - Ap[cc];
    float rsold = dot_compact<F>(r, r);
    bool active = valid && rsold >= 1e-20f;  // else: x untouched (_als.pyx:206)
    const bool store = active;
    for (int it = 0; it + 1 < cg_steps; ++it) {  // all steps but the last; every wave takes the barriers
      publish(p, active);
      if (active && !product_first) tile_pass<F, false, false, false, ST>(y, cw, cnt, prow, sp, lane, 0, ent_col, ent_c, Y);
      product();
      if (active && product_first) tile_pass<F, false, false, false, ST>(y, cw, cnt, prow, sp, lane, 0, ent_col, ent_c, Y);
      __syncthreads();
      collect(Ap);
      if (active) {  // wave-uniform
#pragma unroll
        for (int cc = 0; cc < FC; ++cc) Ap[cc] += sp[cc];
        const float alpha = rsold * __builtin_amdgcn_rcpf(dot_compact<F>(p, Ap));
#pragma unroll
        for (int cc = 0; cc < FC; ++cc) {
          xc[cc] = fmaf(alpha, p[cc], xc[cc]);
          r[cc] = fmaf(-alpha, Ap[cc], r[cc]);
        }
        const float rsnew = dot_compact<F>(r, r);
        if (rsnew < 1e-20f) {
          active = false;  // the oracle breaks here (_als.pyx:235); the wave keeps taking the barriers
        } else {
          const float beta = rsnew * __builtin_amdgcn_rcpf(rsold);
#pragma unroll
          for (int cc = 0; cc < FC; ++cc) p[cc] = fmaf(beta, p[cc], r[cc]);
          rsold = rsnew;
        }
      }
    }
    // last step: only its x update is evaluated (_als.pyx:226-241 compute r, rsnew, p that nothing reads), and that needs the
    // scalar p . A p alone: the tile pass hands in its part as one value per lane, the 16-row product stays as it is; its
    // tile pass rolls the next group's entries in
    bool rolled = false;
    if (cg_steps > 0) {
      publish(p, active);
      float tile_pAp = 0.f;
      auto last_tiles = [&]() {
        if constexpr (ROLL) tile_pAp = tile_pass<F, false, true, true, ST>(y, cw, cnt, prow, sp, lane, ent_cnt, ent_col, ent_c, Y);
        else tile_pAp = tile_pass<F, false, true, false, ST>(y, cw, cnt, prow, sp, lane, 0, ent_col, ent_c, Y);
      };
      if (active && !product_first) last_tiles();
      product();
      if (active && product_first) last_tiles();
      __syncthreads();
      collect(Ap);
      if (active) {
        if constexpr (ROLL) {
          cnt = ent_cnt;
          ent_cnt = row_valid(t2) ? e2 - b2 : 0;
          fetch_entries(indices, data, opaque(lane), b2, max(e2, b2 + 1), ent_col, ent_c);
          load_compact<F>(X + (size_t)id1 * F, opaque(lane), x);
          rolled = true;
        } else {
          kill(x);
        }
        // p . A p = p . (A0 p) + the tile part, in one sum over the wave
        const float alpha = rsold * __builtin_amdgcn_rcpf(wave_allsum(dot_local<FC>(p, Ap) + tile_pAp));
#pragma unroll
        for (int cc = 0; cc < FC; ++cc) xc[cc] = fmaf(alpha, p[cc], xc[cc]);
      } else {
        kill(x);
      }
    } else {
      kill(x);
    }
    if (store) store_compact<F>(xrow, opaque(lane), xc);
    tile_ready = rolled;
    g = t1, t1 = t2, t2 = t3, t3 = t_new;
    id0 = id1, id1 = id2, id2 = id3, id3 = row_id(t3);
    b0 = b1, e0 = e1, b1 = b2, e1 = e2, b2 = indptr[id2], e2 = indptr[id2 + 1];
  }
}

template <int F, typename ST>
__global__ __launch_bounds__(1024) void als_cg_qfgroup_kernel(const int32_t *__restrict__ order, int first, int count,
                                                              const int32_t *__restrict__ indptr,
                                                              const int32_t *__restrict__ indices,
                                                              const float *__restrict__ data, ST *__restrict__ X,
                                                              const ST *__restrict__ Y, const float *__restrict__ A0, int cg_steps) {
  group_stage_gramian<F>(A0);
  group_rows<F, ST>(order, first, count, indptr, indices, data, X, Y, cg_steps);
}

template <typename T>
static void launch_qfgroup(const imp_csr *C, int first, int count, T *X, const T *Y, const float *A0, int cg_steps, const char *name) {
  if (count <= 0) return;
  constexpr int F = 128;
  const size_t lds = QFGroupCfg<F>::lds_bytes;
  auto kern = als_cg_qfgroup_kernel<F, T>;
  allow_dynamic_lds(kern, lds);
  int grid = std::min((count + 15) / 16, ctx().num_cus * std::max(2, ctx().oversub));  // (1 / 2 / 3 per CU measured within 1 %)
  IMP_PROF(name);
  kern<<<grid, 1024, lds, stream()>>>(C->order.data(), first, count, C->indptr.data(), C->indices.data(), C->data.data(), X, Y, A0,
                                      cg_steps);
  IMP_CHECK_HIP(hipGetLastError());
}

// ---- the two 1024-thread classes in one persistent launch ----------------------------------------------------------------
// (256,512] -- a team of 16 wavefronts per row -- and the short rows both hold a CU with one workgroup.  As two launches on a
// grid of two workgroups per CU every CU staged the gramian twice per class (for the short rows: 16 K values split into three
// bf16 planes), started its pipelines twice and idled in two tails.  Here the grid is exactly the resident workgroups; a
// workgroup runs team-16 rows by ticket (team_rows, TICKETS, one team per workgroup), then -- after one barrier -- re-stages the
// gramian as bf16 planes over the same allocation and runs groups of short rows by ticket (group_rows, TICKETS).  The ticket
// bookkeeping is WideTickets (team_tickets.h).  Every row's arithmetic is that of its class kernel.
//
// At its head the launch carries the FIX-UP of the long-row path (long_tail_route.h says when): every launch that can list a row
// has ended behind a kernel boundary, so the count every workgroup reads is complete.  It is normally zero -- one scalar load.
// Otherwise the 16 wavefronts of workgroup b take the listed rows i = 16 b + wave, + 16 grid, ... through cg_fixup_row
// (als_cg_fixup.h) on F floats of LDS each, and one barrier hands the allocation to the classes.
//
// IMP_WIDE_FORM (compile time, A/B builds): 0 the chain with tickets in both classes; 1 the chain with the short rows' groups
// dealt in fixed strides over the resident grid; 2 no chain: each class in a launch of its own on the resident grid, with tickets.
#ifndef IMP_WIDE_FORM
#define IMP_WIDE_FORM 0
#endif
struct WideClassArgs {
  int first[WideTickets::kClasses], count[WideTickets::kClasses];  // rows
  unsigned base[WideTickets::kClasses][WideTickets::kQueues];
};
struct WideFixupArgs {  // the fix list of the long-row path, re-solved at the head of the launch
  const unsigned *count = nullptr, *rows = nullptr;
  int capacity = 0;  // 0: no fix-up in this launch
  unsigned long long *total = nullptr;  // host-mapped: rows re-solved (fixup_total)
};
static_assert(WideTickets::kQueues == kTicketQueues && WideTickets::kGroupRows == 16, "queues and groups of the ticketed classes");
// the larger of the two layouts; the short rows' ticket word follows theirs
template <int F> constexpr size_t wide_chain_lds_bytes() {
  return std::max(team_lds_bytes<F, 16, 1024, 32>(), QFGroupCfg<F>::lds_bytes + 16);
}
template <int F, typename ST, bool SHORT_TICKETS>
__global__ __launch_bounds__(1024) void als_cg_qfwide_chain_kernel(const int32_t *__restrict__ order, WideClassArgs cls,
                                                                   unsigned *__restrict__ counters,
                                                                   const int32_t *__restrict__ indptr,
                                                                   const int32_t *__restrict__ indices,
                                                                   const float *__restrict__ data, ST *__restrict__ X,
                                                                   const ST *__restrict__ Y, const float *__restrict__ A0,
                                                                   int cg_steps, WideFixupArgs fix) {
  if (fix.capacity > 0) {  // uniform over the grid, as is n
    const int n = min((int)fix.count[0], fix.capacity);
    if (n != 0) {
      extern __shared__ __attribute__((aligned(16))) float smem[];
      if (blockIdx.x == 0 && threadIdx.x == 0)
        __hip_atomic_fetch_add(fix.total, (unsigned long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
      for (int i = blockIdx.x * 16 + wave; i < n; i += gridDim.x * 16)
        cg_fixup_row<F, ST>(smem + wave * F, lane, (int)fix.rows[i], indptr, indices, data, X, Y, A0, cg_steps);
      __syncthreads();  // every wavefront has left its operand slot
    }
  }
  const unsigned queue = blockIdx.x % kTicketQueues;
  if (cls.count[0] > 0)  // uniform over the grid
    team_rows<Tile32<ST>, F, 16, 1024, true, true>(order, cls.first[0], cls.count[0], indptr, indices, data, X, Y, A0, cg_steps,
                                                   counters + queue * WideTickets::kCounterStride, cls.base[0][queue]);
  if (cls.count[1] > 0) {
    if (cls.count[0] > 0) __syncthreads();  // every wavefront has left the team layout
    group_stage_gramian<F>(A0);
    group_rows<F, ST, SHORT_TICKETS>(order, cls.first[1], cls.count[1], indptr, indices, data, X, Y, cg_steps,
                                     counters + (kTicketQueues + queue) * WideTickets::kCounterStride, cls.base[1][queue]);
  }
}

template <typename T>
void launch_wide_chain(const imp_csr *C, int f, const int (&first)[2], const int (&count)[2], T *X, const T *Y, const float *A0, int cg_steps,
                       const char *name, const NmTail *fixup) {
  if constexpr (std::is_same<T, float>::value) {
    if (f != 128) throw std::invalid_argument("launch_wide_chain: f must be 128");
    constexpr int F = 128;
    constexpr bool kShortTickets = IMP_WIDE_FORM != 1;
    if (count[0] <= 0 && count[1] <= 0) {
      if (fixup) throw std::logic_error("launch_wide_chain: a fix-up without a launch to carry it");
      return;
    }
    static_assert(16 * F * sizeof(float) <= wide_chain_lds_bytes<F>(), "an operand slot per wavefront of the fix-up");
    WideFixupArgs fix;  // carried by the first launch queued here
    if (fixup && fixup->capacity > 0)
      fix = WideFixupArgs{reinterpret_cast<const unsigned *>(fixup->ctl + 2), fixup->fix_rows, fixup->capacity, fixup_total()};
    const size_t lds = wide_chain_lds_bytes<F>();
    auto kern = als_cg_qfwide_chain_kernel<F, T, kShortTickets>;
    // the resident workgroups per CU, asked of the runtime once per process (registers and LDS allow one)
    static const int per_cu = [&] {
      int n = 0;
      allow_dynamic_lds(kern, lds);
      IMP_CHECK_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void *>(kern), 1024, lds));
      if (n < 1) throw std::runtime_error("launch_wide_chain: the kernel does not fit a compute unit");
      return n;
    }();
    allow_dynamic_lds(kern, lds);
    const int grid = std::max(ctx().num_cus * per_cu, WideTickets::kQueues);  // every queue needs a workgroup
    for (int c = 0; c < 2; ++c)
      if (count[c] >= WideTickets::kMaxCount) throw std::invalid_argument("launch_wide_chain: too many rows in a class");
    Context &cx = ctx();
    // zeroed once, on the library stream
    cx.wide_counters.reserve((size_t)WideTickets::kClasses * WideTickets::kQueues * WideTickets::kCounterStride, true);
    // one launch of the classes in `on`
    auto run = [&](bool on0, bool on1) {
      WideClassArgs cls;
      const int32_t rows[2] = {on0 ? std::max(count[0], 0) : 0, on1 ? std::max(count[1], 0) : 0};
      if (rows[0] == 0 && rows[1] == 0) return;
      for (int c = 0; c < 2; ++c) cls.first[c] = first[c], cls.count[c] = rows[c];
      WideTickets after = cx.wide_tickets;
      // (fixed strides draw nothing: the bases of the short rows are not used and must not move)
      const int32_t ticketed[2] = {rows[0], kShortTickets ? rows[1] : 0};
      after.launch_rows(ticketed, grid, cls.base);
      kern<<<grid, 1024, lds, stream()>>>(C->order.data(), cls, cx.wide_counters.data(), C->indptr.data(), C->indices.data(),
                                         C->data.data(), X, Y, A0, cg_steps, fix);
      IMP_CHECK_HIP(hipGetLastError());
      fix = WideFixupArgs{};
      cx.wide_tickets = after;  // a launch that was not queued draws nothing
    };
    IMP_PROF(name);
    if (IMP_WIDE_FORM == 2) run(true, false), run(false, true);
    else run(true, true);
  } else {
    throw std::invalid_argument("launch_wide_chain: fp32 storage only");
  }
}
template void launch_wide_chain<float>(const imp_csr *, int, const int (&)[2], const int (&)[2], float *, const float *, const float *, int,
                                       const char *, const NmTail *);
template void launch_wide_chain<__half>(const imp_csr *, int, const int (&)[2], const int (&)[2], __half *, const __half *, const float *,
                                        int, const char *, const NmTail *);

template <typename T>
void launch_group_fused(const imp_csr *C, int f, int first, int count, T *X, const T *Y, const float *A0, int cg_steps, const char *name) {
  if (f == 128) launch_qfgroup<T>(C, first, count, X, Y, A0, cg_steps, name);
  else throw std::invalid_argument("launch_group_fused: f must be 128 (f = 64 short rows run on independent wavefronts)");
}
template void launch_group_fused<float>(const imp_csr *, int, int, int, float *, const float *, const float *, int, const char *);
template void launch_group_fused<__half>(const imp_csr *, int, int, int, __half *, const __half *, const float *, int, const char *);

// width: 1 (f = 64 short rows), 2, 4, 8, 16.  float16 storage comes here for the f = 64 short rows only: its mid rows run on the
// packed tiles (als_cg_qh.hip), its f = 128 short rows on the group kernel.
template <typename T>
void launch_team_fused(const imp_csr *C, int f, int width, int first, int count, T *X, const T *Y, const float *A0, int cg_steps,
                       const char *name) {
  if constexpr (std::is_same<T, __half>::value) {
    if (f != 64 || width != 1) throw std::invalid_argument("launch_team_fused: float16 storage takes the f = 64 short rows only");
    launch_qfteam<64, 1, 512, T>(C, first, count, X, Y, A0, cg_steps, name);
  } else {
    auto run = [&](auto Fc) {
      constexpr int F = decltype(Fc)::value;
      switch (width) {
        case 16: launch_qfteam<F, 16, 1024, T>(C, first, count, X, Y, A0, cg_steps, name); break;
        case 8: launch_qfteam<F, 8, 512, T>(C, first, count, X, Y, A0, cg_steps, name); break;
        case 4: launch_qfteam<F, 4, 512, T>(C, first, count, X, Y, A0, cg_steps, name); break;
        case 2: launch_qfteam<F, 2, 512, T>(C, first, count, X, Y, A0, cg_steps, name); break;
        case 1:
          if constexpr (F == 64) launch_qfteam<F, 1, 512, T>(C, first, count, X, Y, A0, cg_steps, name);
          else throw std::invalid_argument("launch_team_fused: one wave per row needs f = 64");
          break;
        default: throw std::invalid_argument("launch_team_fused: team width");
      }
    };
    if (f == 128) run(idx_t<128>{});
    else if (f == 64) run(idx_t<64>{});
    else throw std::invalid_argument("launch_team_fused: f must be 64 or 128");
  }
}
template void launch_team_fused<float>(const imp_csr *, int, int, int, int, float *, const float *, const float *, int, const char *);
template void launch_team_fused<__half>(const imp_csr *, int, int, int, int, __half *, const __half *, const float *, int,
                                        const char *);

}  // namespace imp
