// K1t: the mid-row CG half sweep at f = 64 / 128 -- a team of WPR wavefronts per row, the whole row resident in registers for
// all 1 + cg_steps passes (team_rows below) -- and its building blocks.  One body, two tile policies: 32-entry fp32 tiles
// (Tile32, als_cg_qf.hip; fp16 storage converted at the load) and 64-entry tiles of packed halves widened inside the FMA
// (Tile64, als_cg_qh.hip).  als_cg_q.hip has the dispatch over the row classes.
//
// Arithmetic contract: the oracle's CG (implicit/cpu/_als.pyx:152-248).
//
// What the round-2 team kernels spent (profiles/micro/valu_rate.hip, profiles/r04_micro_valu_rate.txt; HISTORY.md section 4.1 has
// the full picture): saturated, a SIMD retires a plain vector instruction every 2.3 cycles and a packed FMA, a DPP form or an
// SGPR-operand form every 4.1-4.4; one wave alone issues only every 5.5-6 cycles.  The round-2 kernels executed 1.03 G vector
// instructions per C3 iteration for the mid-row classes, and only ~55 % of them were the FMAs of the dense part and of the tile;
// the rest was per-wavefront bookkeeping, REPLICATED in every wavefront of a team:
//   - the CG scalars (two wave-wide dot reductions, two IEEE divisions, the x / r / p updates) -- every wave of a team
//     did the identical arithmetic on identical bits;
//   - the operand's expansion from the compact to the quarter layout (6 v_permlane swaps + 12 register copies per pass)
//     and the sum of the team's partial vectors in every wave.
// (A first version of the micro-benchmark, run on a box in a low-power state, read 7.5 cycles for everything and led to the
// conclusion "100 % issue bound"; the instruction count was worth cutting anyway: 808 M now.)
// Round 3 gives that work to ONE wavefront per team (the leader, sub == 0) and turns the rest into LDS traffic, which
// has issue slots of its own:
//   * the leader alone sums the team's partial vectors, does the CG update and PUBLISHES the next operand in LDS (natural
//     factor order) together with a go / last / stop word; the other waves wait on the team's generation counter (an idle
//     wave costs no issue slots -- that is the point) and read the operand back already expanded: two ds_read_b128 per
//     lane, no swaps.  Two counters per team (arrivals A, generation B), no workgroup barrier after the prologue;
//   * a / b by v_rcp_f32 (1 ulp) instead of the 12-instruction IEEE sequence; the last CG step only updates x, and for that
//     it needs the scalar p . A p alone: its pass keeps the tile's dots and drops the weight broadcasts, the axpys, the
//     reduce-scatter and the partial VECTOR -- a wave hands the leader one float (fused_pass, LAST);
//   * the dots of a pair of tile steps are reduced together (5 DPP adds for two values instead of 8) and the weight is
//     applied straight from the lane that holds the total (row_newbcast operand of the multiply);
//   * per-entry weights |c| - 1 and c+ live in an LDS table written once per row (gather_pair).
// Kept from the first round-3 version: fused passes (the gramian rows of a pass are dealt to 4 ticks per pair of tile steps
// whose LDS reads are issued before a tile half-step and consumed after it) and the rolling gather (the last pass of a row
// re-fills each pair of tile registers with the next row's entries as soon as the pair is done; metadata runs ids 4 rows ahead,
// nnz ranges 3, entries 2).
#ifndef IMPLICIT_AMD_CSRC_ALS_QF_COMMON_H_
#define IMPLICIT_AMD_CSRC_ALS_QF_COMMON_H_
#include <type_traits>
#include <utility>

#include "als_qtile.h"

namespace imp {

// The compiler hoists everything derived from the lane id out of the row loop (byte offsets, 64-bit gather bases, LDS
// addresses: a dozen registers) and then spills it, because the tile fills the file.  Lane-derived values are therefore
// re-derived where they are used, from a copy of the lane id the optimiser cannot see through.
__device__ __forceinline__ int opaque(int v) {
  asm volatile("" : "+v"(v));
  return v;
}

// explicit packed math: pairs of adjacent expanded slots travel as one 64-bit register pair (v_pk_fma_f32); left to the
// SLP vectoriser the dots came out as scalar v_fmac chains once the operand arrived by ds_read_b128
typedef float f32x2 __attribute__((ext_vector_type(2)));

template <int I> using idx_t = std::integral_constant<int, I>;
template <int N, typename Fn, int... Is> __device__ __forceinline__ void static_for_impl(Fn &&fn, std::integer_sequence<int, Is...>) {
  (fn(idx_t<Is>{}), ...);
}
template <int N, typename Fn> __device__ __forceinline__ void static_for(Fn &&fn) {
  static_for_impl<N>(fn, std::make_integer_sequence<int, N>{});
}

// The gramian rows of one wave and pass dealt to TICKS ticks, four per pair of tile steps.  The wave's F / WPR rows are cut
// into four runs of NJ consecutive rows, one per 16-lane group: step s of group g is row j_begin + g NJ + s, so a group's
// operand entries p_j are consecutive and travel two at a time (ds_read_b64 costs the LDS the same two cycles as a b32).
// One step = FE/4 ds_read_b128 in flight per tick (8 registers at f = 128) + the operand pair.
template <int F, int NJ, int TICKS> struct DenseTicks {
  static constexpr int FE = F / 16, Q4 = FE / 4;
  static constexpr int EVERY = TICKS / NJ;  // ticks K with K % EVERY == 0 carry one step
  static_assert(NJ >= 1 && NJ <= TICKS && TICKS % NJ == 0 && (NJ & (NJ - 1)) == 0, "steps per pass");
  float4 a[Q4];
  f32x2 vj2;
  template <int K> __device__ __forceinline__ void issue(const float *row, const float *vp) {
    if constexpr (K % EVERY == 0) {
      constexpr int s = K / EVERY;
      if constexpr (NJ == 1) vj2 = f32x2{vp[0], 0.f};
      else if constexpr (s % 2 == 0) vj2 = *reinterpret_cast<const f32x2 *>(vp + s);
#pragma unroll
      for (int e = 0; e < Q4; ++e) a[e] = *reinterpret_cast<const float4 *>(row + (size_t)s * F + 64 * e);
    }
  }
  template <int K> __device__ __forceinline__ void consume(f32x2 (&ae)[FE / 2]) {
    if constexpr (K % EVERY == 0) {
      constexpr int s = K / EVERY;
      const float vj = (s % 2 == 0) ? vj2.x : vj2.y;
      const f32x2 v2 = {vj, vj};
#pragma unroll
      for (int e = 0; e < Q4; ++e) {
        ae[2 * e] = __builtin_elementwise_fma(v2, f32x2{a[e].x, a[e].y}, ae[2 * e]);
        ae[2 * e + 1] = __builtin_elementwise_fma(v2, f32x2{a[e].z, a[e].w}, ae[2 * e + 1]);
      }
    }
  }
};

// the dots of two tile steps, reduced over the 16 lanes of each group TOGETHER: after the first level the lower half-row
// carries d0's pair sums and the upper half d1's, the remaining three levels (half-row mirror, quad xor 1, quad xor 2: all
// inside a half-row) then serve both.  Lanes 0-7 of every row end with the total of d0, lanes 8-15 with the total of d1.
__device__ __forceinline__ float reduce_pair(float d0, float d1) {
  float u = d1 + dpp_mov<0x128>(d1);  // row_ror:8
  const float s0 = d0 + dpp_mov<0x128>(d0);
  u = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, u), __builtin_bit_cast(int, s0), 0xE4, 0xF, 0x3,
                                                            false));  // quad_perm:[0,1,2,3] into banks 0, 1 = lanes 0-7
  u += dpp_mov<0x141>(u);  // row_half_mirror
  u += dpp_mov<0xB1>(u);   // quad_perm:[1,0,3,2]
  u += dpp_mov<0x4E>(u);   // quad_perm:[2,3,0,1]
  return u;
}
template <int LANE> __device__ __forceinline__ float row_bcast_from(float v) {  // row_newbcast:LANE (gfx90a+)
  return dpp_mov<0x150 + LANE>(v);
}

// queues of a ticketed row class (team_tickets.h ChainTickets::kQueues)
constexpr int kTicketQueues = 8;

// control word the leader publishes with every operand
enum : unsigned { kGo = 1u, kLast = 2u };

// tunables of the team protocol (compile-time: s_sleep / s_setprio take immediates; -D overrides for A/B builds,
// implicit_amd/_build.py build_variant)
#ifndef IMP_TEAM_NAP_FIRST
#define IMP_TEAM_NAP_FIRST 6   // a worker's first nap while the leader updates (64-cycle units)
#endif
#ifndef IMP_TEAM_NAP_NEXT
#define IMP_TEAM_NAP_NEXT 2    // its later naps
#endif
#ifndef IMP_TEAM_NAP_LEADER
#define IMP_TEAM_NAP_LEADER 1  // the leader's naps while it waits for the arrivals
#endif
#ifndef IMP_TEAM_LEADER_PRIO
#define IMP_TEAM_LEADER_PRIO 0 // wave priority of a leader from "arrivals complete" to "operand published" (the team idles meanwhile)
#endif

// ---- the team kernel, written against a tile policy `Tile` --------------------------------------------------------------
//   Tile::T          entries per wavefront, 4 per tile step (entry t = 4 q + g belongs to 16-lane group g): T / 8 pairs of
//                    steps, 4 dense ticks per pair; a wave's weight table holds |c| - 1 at cw[t] and c+ at cw[T + t]
//   Tile::ROLL       the last pass of a row gathers the next row's tile (rolling gather)
//   Tile::elem       one register of an entry's slice: its expanded slots 2 h and 2 h + 1
//   Tile::fetch      stages the (column, confidence) pairs of a slice, entry t in lane t
//   Tile::gather<H>  an entry's H elements from its factor row;  dot<H>: this lane's share of y . v;  axpy<H>: ae += w y
// The products associate alike in both policies: even expanded slots in one running sum, odd slots in the other.

// Entries of tile steps 2 P and 2 P + 1.  The staged registers hold entry min(t, cnt - 1) of the wave's slice in lane t
// (Tile::fetch): the gather addresses travel by ds_bpermute (entry t = 4 q + g -> the 16 lanes of group g), the two
// weights every pass derives from a confidence -- |c| - 1 and c+ = max(c, 0), both 0 for the padding entries -- are written
// ONCE to a wave-private LDS table by the lanes that hold the entries and read back per step as a group-wide broadcast:
// 8 registers less than carrying them, and no per-pass abs / max.
template <typename Tile, int F, int P, typename ST>
__device__ __forceinline__ void gather_pair(typename Tile::elem (&y)[Tile::T / 4][F / 32], float *cw, int col_reg, float c_reg, int cnt,
                                            const ST *__restrict__ Y, int lane) {
  lane = opaque(lane);
  if ((lane >> 3) == P) {  // lanes 8 P .. 8 P + 7 hold the entries of this pair
    const bool ok = lane < cnt;
    cw[lane] = ok ? fabsf(c_reg) - 1.f : 0.f;
    cw[Tile::T + lane] = ok ? fmaxf(c_reg, 0.f) : 0.f;
  }
  const int src = 4 * (lane >> 4);  // byte address of the source lane
#pragma unroll
  for (int q = 2 * P; q < 2 * P + 2; ++q) {
    const unsigned col = (unsigned)__builtin_amdgcn_ds_bpermute(src + 16 * q, col_reg);
    Tile::template gather<F / 32>(y[q], Y + (size_t)col * F + 4 * (lane & 15));
  }
}

// One pass over this wave's share of a row: acc (compact) = [its gramian rows] . v  +  [its tile entries] weights, v being
// the operand the team's leader published in LDS (`vt`, natural factor order).
//   FIRST: v = x, weights c+ - (|c|-1) y.x, the dense part enters negated (_als.pyx:187-201): the pass accumulates
//          A0 x - sum w y and the caller takes the sum of the team's partials with a minus sign
//   else : weights (|c|-1) y.v (_als.pyx:214-222)
//   LAST : v = p of the row's last CG step, which needs alpha = rsold / (p . A p) and nothing else of A p.  The pass forms
//          no vector: it RETURNS this wave's share of the scalar (the same value in every lane; acc is left alone),
//              p . A p = p . (A0 p) + sum_k (|c_k|-1) (y_k . p)^2,
//          i.e. the tile entries keep their dots and lose the weight broadcasts and the axpys, the dense ticks accumulate
//          their gramian rows as in every pass and are dotted with the operand at the end.
//   ROLL : the tile registers (and weight-table slots) of pair P are re-filled with the next row's entries once the pair is
//          done (with LAST only)
template <typename Tile, int F, int NJ, bool FIRST, bool LAST, bool ROLL, typename ST>
__device__ __forceinline__ float fused_pass(typename Tile::elem (&y)[Tile::T / 4][F / 32], float *cw, int cnt, const float *vt,
                                            int j_begin, const float *A0s, float (&acc)[F / 64], int lane, int cnt_nx, int &col_nx,
                                            float &c_nx, const ST *__restrict__ Y, const int32_t *__restrict__ indices,
                                            const float *__restrict__ data, int k0_nx2, int end_nx2) {
  static_assert(!(FIRST && LAST) && (LAST || !ROLL), "pass form");
  constexpr int FE = F / 16, H = FE / 2, PAIRS = Tile::T / 8;
  if constexpr (ROLL) {
    // The staged entries were requested a row ago.  Passing them through an opaque copy makes the compiler wait for them
    // HERE, once, while nothing else is in flight; without it every use inside the pass would wait for "all loads so far"
    // (vmcnt(0): its counter bookkeeping does not survive the branches of the pass) -- i.e. for the rolling gathers of
    // the pairs before.
    col_nx = opaque(col_nx);
    c_nx = __int_as_float(opaque(__float_as_int(c_nx)));
  }
  f32x2 ve[H], ae[H];
  const float *row, *vp, *cwg;
  {
    const int ln = opaque(lane);
    const int g = ln >> 4, m = ln & 15;
#pragma unroll
    for (int e = 0; e < FE; e += 4) {  // the operand, expanded: slot e of lane (g, m) is factor 64 (e / 4) + 4 m + (e & 3)
      const float4 t = *reinterpret_cast<const float4 *>(vt + 16 * e + 4 * m);
      ve[e / 2] = f32x2{t.x, t.y}, ve[e / 2 + 1] = f32x2{t.z, t.w};
    }
    vp = vt + j_begin + g * NJ;
    row = A0s + (size_t)(j_begin + g * NJ) * F + 4 * m;
    cwg = cw + g;  // this group's entries: t = 4 q + g
    // LAST: reduce_pair leaves the dot of step 2 P in lanes 0-7 of a row and that of step 2 P + 1 in lanes 8-15: every
    // lane reads the one weight that belongs to the total it holds
    if constexpr (LAST) cwg += 4 * (m >> 3);
  }
#pragma unroll
  for (int h = 0; h < H; ++h) ae[h] = f32x2{0.f, 0.f};
  float s8 = 0.f;  // LAST: sum of (|c|-1) (y . p)^2 over this lane's totals; every entry is counted in 8 lanes
  DenseTicks<F, NJ, 4 * PAIRS> dt;
  auto partial = [&](int q) { return Tile::template dot<H>(y[q], ve); };
  auto axpy = [&](int q, float w) { Tile::template axpy<H>(y[q], w, ae); };
  static_for<PAIRS>([&](auto Pc) {
    constexpr int P = decltype(Pc)::value;
    if (8 * P < cnt) {  // wave-uniform
      dt.template issue<4 * P>(row, vp);
      const float cm1_0 = cwg[8 * P];
      float cm1_1 = 0.f, cp_0 = 0.f, cp_1 = 0.f;
      if constexpr (!LAST) cm1_1 = cwg[8 * P + 4];
      if constexpr (FIRST) cp_0 = cwg[Tile::T + 8 * P], cp_1 = cwg[Tile::T + 8 * P + 4];
      __builtin_amdgcn_sched_barrier(0);
      const float d0 = partial(2 * P);
      __builtin_amdgcn_sched_barrier(0);
      dt.template consume<4 * P>(ae);
      dt.template issue<4 * P + 1>(row, vp);
      __builtin_amdgcn_sched_barrier(0);
      const float d1 = partial(2 * P + 1);
      if constexpr (LAST) {
        // the third tick's LDS reads have the reduction to hide behind
        __builtin_amdgcn_sched_barrier(0);
        dt.template consume<4 * P + 1>(ae);
        dt.template issue<4 * P + 2>(row, vp);
        __builtin_amdgcn_sched_barrier(0);
        // no fence between the reduction and the packed FMAs of the tick: they fill the wait states of its dependent DPP chain
        const float u = reduce_pair(d0, d1);
        s8 = fmaf(cm1_0 * u, u, s8);
        dt.template consume<4 * P + 2>(ae);
        __builtin_amdgcn_sched_barrier(0);
        dt.template issue<4 * P + 3>(row, vp);
        __builtin_amdgcn_sched_barrier(0);
        dt.template consume<4 * P + 3>(ae);
      } else {
        // no fence between the reduction and the packed FMAs of the tick: they fill the wait states of its dependent DPP chain
        const float u = reduce_pair(d0, d1);
        dt.template consume<4 * P + 1>(ae);
        // the whole first pass is accumulated negated: w' = (|c|-1) d - c+
        const float w0 = FIRST ? fmaf(cm1_0, row_bcast_from<0>(u), -cp_0) : cm1_0 * row_bcast_from<0>(u);
        const float w1 = FIRST ? fmaf(cm1_1, row_bcast_from<8>(u), -cp_1) : cm1_1 * row_bcast_from<8>(u);
        __builtin_amdgcn_sched_barrier(0);
        dt.template issue<4 * P + 2>(row, vp);
        __builtin_amdgcn_sched_barrier(0);
        axpy(2 * P, w0);
        __builtin_amdgcn_sched_barrier(0);
        dt.template consume<4 * P + 2>(ae);
        dt.template issue<4 * P + 3>(row, vp);
        __builtin_amdgcn_sched_barrier(0);
        axpy(2 * P + 1, w1);
        __builtin_amdgcn_sched_barrier(0);
        dt.template consume<4 * P + 3>(ae);
      }
    } else {  // no entries left: the remaining gramian rows
      // (the empty statement keeps the two branches from starting alike: the compiler otherwise hoists "read, wait,
      // consume" of the first tick above the branch and the tick's LDS latency is exposed again)
      asm volatile("" ::: "memory");
      static_for<4>([&](auto Kc) {
        constexpr int K = 4 * P + decltype(Kc)::value;
        dt.template issue<K>(row, vp);
        __builtin_amdgcn_sched_barrier(0);
        dt.template consume<K>(ae);
      });
    }
    if constexpr (ROLL) {
      if (8 * P < cnt_nx) gather_pair<Tile, F, P>(y, cw, col_nx, c_nx, cnt_nx, Y, lane);
    }
    __builtin_amdgcn_sched_barrier(0);
  });
  float pAp = 0.f;
  if constexpr (LAST) {
    // this wave's gramian rows: sum_j p_j (A0 p)_j = sum over the lanes of ae . ve, in Tile::dot's even / odd association;
    // the tile part enters with the exact scale 1/8 that undoes its eightfold count
    f32x2 t = ae[0] * ve[0];
#pragma unroll
    for (int h = 1; h < H; ++h) t = __builtin_elementwise_fma(ae[h], ve[h], t);
    pAp = wave_allsum(fmaf(0.125f, s8, t.x + t.y));
  } else {
    float aes[FE];
#pragma unroll
    for (int h = 0; h < H; ++h) aes[2 * h] = ae[h].x, aes[2 * h + 1] = ae[h].y;
    reduce_expanded<F>(aes, acc);
  }
  if constexpr (ROLL) {
    // the staged entries are used up: stage those of the row after the next (loads complete in order: before the leader's
    // request for the next row's iterate, which is the first thing the next row waits for)
    Tile::fetch(indices, data, opaque(lane), k0_nx2, end_nx2, col_nx, c_nx);
  }
  return pAp;
}

// dynamic LDS of team_rows, in bytes: gramian [F][F], partial vectors [WAVES][F], operands [TEAMS][F], weight tables
// [WAVES][2 T], control words [TEAMS][4]
template <int F, int WPR, int BLOCK, int T> constexpr size_t team_lds_bytes() {
  constexpr size_t WAVES = BLOCK / 64, TEAMS = WAVES / WPR;
  return ((size_t)F * F + WAVES * F + TEAMS * F + 2 * T * WAVES + 4 * TEAMS) * sizeof(float);
}

// A team kernel has three parts: a workgroup prologue (the gramian image into LDS), a per-class set-up (the teams' control
// words, one barrier) and the row loop.  A kernel of one row class runs them in sequence (team_rows with its defaults: the
// body of als_cg_qfteam_kernel, Tile32, and als_cg_q64team_kernel, Tile64); the chain kernel of the three 512-thread classes
// (als_cg_qfteam_chain_kernel, als_cg_qf.hip) runs the prologue once, here, and then set-up and row loop per class (STAGE false).
template <int F, int BLOCK> __device__ __forceinline__ void team_stage_gramian(const float *__restrict__ A0) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  for (int e = threadIdx.x; e < F * F; e += BLOCK) smem[e] = A0[e];  // no barrier: the first class set-up has one
}

// One row class: rows [first, first + count) of the schedule, a team of WPR wavefronts per row, up to T WPR nonzeros per row
// -- the (prologue,) set-up and the row loop.
//   STAGE   false: the gramian image is in LDS already (at the start of the allocation, whatever the team width).
//   TICKETS false: a team's rows are i = (blockIdx.x + k gridDim.x) TEAMS + team -- the per-class kernels.
//   TICKETS true : a team draws its rows by ticket (team_tickets.h has the arithmetic).  The class is dealt to eight queues
//     (one counter per queue; `counter` and `base` are those of this workgroup's): with N teams on a queue, team g starts
//     with the tickets g, g + N, g + 2 N, g + 3 N -- the four rows the metadata pipeline holds -- and every later one is an
//     atomic increment of *counter (tickets from 4 N on: counter - base + 4 N).  The leader draws at the top of a row,
//     where nothing else of its wave is in flight, takes the value after the row's first pass and hands it to the team in
//     the upper 30 bits of the row's STOP word -- the one control word of a row every wavefront reads last, on every path.
//     No wavefront waits or polls for a ticket.  Tickets at or past the queue's end (clamped to it) behave like the clamped
//     indices of the other mode; a team that holds one stops drawing.
template <typename Tile, int F, int WPR, int BLOCK, bool TICKETS = false, bool STAGE = true, typename ST>
__device__ __forceinline__ void team_rows(const int32_t *__restrict__ order, int first, int count, const int32_t *__restrict__ indptr,
                                          const int32_t *__restrict__ indices, const float *__restrict__ data, ST *__restrict__ X,
                                          const ST *__restrict__ Y, const float *__restrict__ A0, int cg_steps,
                                          unsigned *counter = nullptr, unsigned base = 0u) {
  constexpr int FC = F / 64, FE = F / 16, T = Tile::T, WAVES = BLOCK / 64, TEAMS = WAVES / WPR, NJ = F / WPR / 4;
  static_assert(WPR <= WAVES && (F / WPR) % 4 == 0, "team width");
  static_assert(!TICKETS || WPR > 1, "tickets travel in the team protocol");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *A0s = smem;                            // [F][F]
  float *parts = A0s + (size_t)F * F;           // [WAVES][F]  partial vectors of the waves (compact slots at their natural index)
  float *vts = parts + (size_t)WAVES * F;       // [TEAMS][F]  the operand the leader published (natural factor order)
  float *cws = vts + (size_t)TEAMS * F;         // [WAVES][2 T]  per-entry weights |c| - 1 and c+ of the resident tile (gather_pair)
  unsigned *ctl = reinterpret_cast<unsigned *>(cws + (size_t)WAVES * 2 * T);  // [TEAMS][4]  arrivals A, generation B, control words
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int team = wave / WPR, sub = wave % WPR;
  const bool leader = sub == 0;
  if constexpr (STAGE) {  // workgroup prologue (team_stage_gramian)
    for (int e = threadIdx.x; e < F * F; e += BLOCK) A0s[e] = A0[e];
  }
  // per-class set-up: the control words start at zero
  if (threadIdx.x < 4 * TEAMS) ctl[threadIdx.x] = 0u;
  __syncthreads();  // the only workgroup-wide barrier of a class: from here on the teams run their rows independently
  const int j_begin = F * sub / WPR;
  float *vt = vts + (size_t)team * F;
  float *cw = cws + (size_t)wave * 2 * T;
  unsigned *arrivals = ctl + 4 * team, *generation = arrivals + 1, *words = arrivals + 2;

  // ---- team protocol ---------------------------------------------------------------------------------------------------
  // worker (every wave, the leader included): wait for generation g -> read word + operand -> pass -> partial to LDS -> arrive
  // leader: wait for WPR arrivals -> sum the partials in wave order -> CG update -> operand + word to LDS -> generation + 1
  // Both counters are monotonic; a wave's LDS operations execute in order, so a partial is in place before its arrival is
  // counted and an operand before its generation is.  The operand slot and the partial slots are single-buffered: the
  // leader overwrites the operand only after all WPR arrivals of the pass that read it, and a wave overwrites its partial
  // only after the next generation, which the leader publishes after having summed it.  The control word has two slots
  // (generation parity): a "stop" generation expects no arrivals, so the leader may publish the next row's first generation
  // before a slow wave has read the stop word -- but never a second one, which needs that wave's arrival.
  unsigned gen = 0, pub = 0, arr_target = 0;
  // LDS byte offsets (the low half of a flat LDS address is the offset inside the workgroup's allocation)
  auto lds_off = [](const void *ptr) { return (unsigned)(size_t)ptr; };
  const unsigned arrivals_off = lds_off(arrivals), generation_off = lds_off(generation), words_off = lds_off(words);
  // the one lane-derived value that stays in a register for the whole kernel: byte offset of this lane's compact slots
  // inside a natural-order vector (the other lane-derived addresses are rebuilt where they are used)
  const unsigned cf4 = 4u * (unsigned)QL<F>::cfactor(lane, 0);
  // The counters are bumped with a bare ds_add_u32 from lane 0: the LDS executes a wave's operations in order, so the
  // partial vector / operand written just before is in place when the counter moves -- no release fence (s_waitcnt), and
  // none of the lane-counting code the compiler wraps around an atomic add inside a divergent branch.
  auto publish = [&](unsigned w) {  // leader
    ++pub;
    if (lane == 0)
      asm volatile("ds_write_b32 %0, %1\n\tds_add_u32 %2, %3" ::"v"(words_off + 4u * (pub & 1u)), "v"(w), "v"(generation_off), "v"(1u)
                   : "memory");
    if constexpr (IMP_TEAM_LEADER_PRIO > 0) __builtin_amdgcn_s_setprio(0);
  };
  auto poll = [&](unsigned off) {  // one ds_read_b32 of a counter, made wave-uniform
    typedef __attribute__((address_space(3))) volatile unsigned lds_word;
    return (unsigned)__builtin_amdgcn_readfirstlane(*(lds_word *)(size_t)off);
  };
  auto await_operand = [&]() -> unsigned {  // every wave; returns the control word
    ++gen;
    if constexpr (WPR > 1) {
      // every poll costs two vector-issue slots (address + readfirstlane): the first nap covers most of the leader's update
      if (poll(generation_off) < gen) {
        __builtin_amdgcn_s_sleep(IMP_TEAM_NAP_FIRST);
        while (poll(generation_off) < gen) __builtin_amdgcn_s_sleep(IMP_TEAM_NAP_NEXT);
      }
    }
    return poll(words_off + 4u * (gen & 1u));
  };
  auto arrive = [&](const float (&acc)[FC]) {  // every wave: partial vector to LDS, then count the arrival
    float *slot = reinterpret_cast<float *>(reinterpret_cast<char *>(parts + (size_t)wave * F) + cf4);
    if constexpr (FC == 2) *reinterpret_cast<float2 *>(slot) = make_float2(acc[0], acc[1]);
    else slot[0] = acc[0];
    if constexpr (WPR > 1) {
      if (lane == 0) asm volatile("ds_add_u32 %0, %1" ::"v"(arrivals_off), "v"(1u) : "memory");
    }
  };
  auto collect = [&](float (&acc)[FC]) {  // leader: wait for the team, sum its partials in wave order
    arr_target += WPR;
    if constexpr (WPR > 1) {
      while (poll(arrivals_off) < arr_target) __builtin_amdgcn_s_sleep(IMP_TEAM_NAP_LEADER);
    }
    if constexpr (IMP_TEAM_LEADER_PRIO > 0) __builtin_amdgcn_s_setprio(IMP_TEAM_LEADER_PRIO);
    const float *slot = reinterpret_cast<const float *>(reinterpret_cast<const char *>(parts + (size_t)(team * WPR) * F) + cf4);
#pragma unroll
    for (int c = 0; c < FC; ++c) acc[c] = 0.f;
#pragma unroll
    for (int w = 0; w < WPR; ++w) {
      if constexpr (FC == 2) {
        const float2 t = *reinterpret_cast<const float2 *>(slot + (size_t)w * F);
        acc[0] += t.x, acc[1] += t.y;
      } else {
        acc[0] += slot[(size_t)w * F];
      }
    }
  };
  // The last pass of a row hands in one float per wave (fused_pass, LAST), in the first word of the wave's partial slot.
  auto arrive_scalar = [&](float v) {  // every wave
    if constexpr (WPR > 1) {
      if (lane == 0)
        asm volatile("ds_write_b32 %0, %1\n\tds_add_u32 %2, %3" ::"v"(lds_off(parts + (size_t)wave * F)), "v"(v), "v"(arrivals_off), "v"(1u)
                     : "memory");
    }
  };
  auto collect_scalar = [&](float own) -> float {  // leader: wait for the team, sum its scalars in wave order
    arr_target += WPR;
    if constexpr (WPR > 1) {
      while (poll(arrivals_off) < arr_target) __builtin_amdgcn_s_sleep(IMP_TEAM_NAP_LEADER);
      asm volatile("" ::: "memory");  // the words below were written by inline assembly: no read of them moves above the wait
      if constexpr (IMP_TEAM_LEADER_PRIO > 0) __builtin_amdgcn_s_setprio(IMP_TEAM_LEADER_PRIO);
      const float *slot = parts + (size_t)(team * WPR) * F;  // uniform addresses: every lane reads the same WPR words
      float sum = 0.f;
#pragma unroll
      for (int w = 0; w < WPR; ++w) sum += slot[(size_t)w * F];
      return sum;
    } else {
      return own;
    }
  };
  auto operand_slot = [&]() { return reinterpret_cast<float *>(reinterpret_cast<char *>(vt) + cf4); };
  auto put_operand = [&](const float (&v)[FC]) {  // leader: compact -> natural order in the team's operand slot
    float *slot = operand_slot();
    if constexpr (FC == 2) *reinterpret_cast<float2 *>(slot) = make_float2(v[0], v[1]);
    else slot[0] = v[0];
  };
  auto get_operand = [&](float (&v)[FC]) {  // leader: the operand is still in its slot -- no registers across the pass
    const float *slot = operand_slot();
    if constexpr (FC == 2) {
      const float2 t = *reinterpret_cast<const float2 *>(slot);
      v[0] = t.x, v[1] = t.y;
    } else {
      v[0] = slot[0];
    }
  };

  // this team's rows: i = (blockIdx.x + k gridDim.x) TEAMS + team, or its tickets; rows past the end re-read the last row
  // TICKETS: the class is dealt to kTicketQueues queues, row k of the class to queue k mod 8, and the workgroups of queue q
  // (blockIdx.x mod 8 = q: one XCD) share its rows; `rows`, the tickets and the team numbering are the queue's
  const int queue = TICKETS ? (int)(blockIdx.x % kTicketQueues) : 0;
  const int rows = TICKETS ? (count - queue + kTicketQueues - 1) / kTicketQueues : count;
  auto row_id = [&](int i) {  // uniform address: scalar load
    return order[first + min(TICKETS ? kTicketQueues * i + queue : i, count - 1)];
  };
  const int i_step = TICKETS ? (int)((gridDim.x - queue + kTicketQueues - 1) / kTicketQueues) * TEAMS : gridDim.x * TEAMS;
  const int i_first = TICKETS ? (int)(blockIdx.x / kTicketQueues) * TEAMS + team : blockIdx.x * TEAMS + team;
  // TICKETS: the tickets of the three rows after the one at the top of the body (the loop variable holds that one's), the
  // ticket the leader has drawn for the team this row (clamped to `rows`), and the counter value of a draw on its way
  int t1 = i_first + i_step, t2 = i_first + 2 * i_step, t3 = i_first + 3 * i_step;
  unsigned drawn_ticket = (unsigned)rows, drawn = 0u;
  // One global atomic from lane 0 of the leader, written out for the reason the LDS counters are (publish): the compiler's
  // form counts lanes first.  Its result is waited for in take_draw, a pass later; until then the compiler knows of no load
  // in flight, and a wait it places for loads of its own can only wait longer for it.
  auto draw = [&]() {
    if (lane == 0) asm volatile("global_atomic_add %0, %1, %2, off sc0" : "=v"(drawn) : "v"(counter), "v"(1u) : "memory");
  };
  auto take_draw = [&]() {
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(drawn)::"memory");
    drawn_ticket = min((unsigned)__builtin_amdgcn_readfirstlane(drawn) - base + 4u * (unsigned)i_step, (unsigned)rows);
  };
  auto stop_word = [&]() -> unsigned { return TICKETS ? drawn_ticket << 2 : 0u; };  // leader: go and last clear
  auto slice = [&](int rb, int re, int &k0, int &cnt) {  // even shares rounded up to whole 4-entry tile steps
    const int chunk = min(T, (((re - rb) + WPR - 1) / WPR + 3) & ~3);
    k0 = min(rb + chunk * sub, re);
    cnt = min(chunk, re - k0);
  };
  // dependent loads per row: schedule entry -> row id -> nnz range -> entries -> factor rows; each stage runs one row further
  // ahead than the next: ids 4 rows, ranges 3, entries 2 (1 when the tile was not rolled in), factor rows 1 (rolled) or 0
  int id0 = row_id(i_first), id1 = row_id(i_first + i_step), id2 = row_id(i_first + 2 * i_step), id3 = row_id(i_first + 3 * i_step);
  int b0 = indptr[id0], e0 = indptr[id0 + 1], b1 = indptr[id1], e1 = indptr[id1 + 1], b2 = indptr[id2], e2 = indptr[id2 + 1];
  // ent_*: staged entries (one per lane) of the next row whose tile has to be gathered
  int ent_col, ent_cnt, k0;
  float ent_c;
  slice(b0, e0, k0, ent_cnt);
  Tile::fetch(indices, data, opaque(lane), k0, max(k0 + ent_cnt, b0 + 1), ent_col, ent_c);
  // x is only meaningful between a load and the top of the next row; every other path overwrites it, so that the compiler
  // does not carry (and spill) the old value across the passes
  auto kill = [](float (&v)[FC]) {
#pragma unroll
    for (int cc = 0; cc < FC; ++cc) v[cc] = 0.f;
  };
  bool tile_ready = false;  // the tile (and, in the leader, the iterate) of the row at the top of the body are on their way
  int cnt = 0;
  typename Tile::elem y[T / 4][FE / 2];  // the resident tile
  float x[FC];  // x: the leader's loop-carried iterate registers (the last step loads the NEXT row's into them)
  kill(x);
  for (int i = i_first; i < rows; i += TICKETS ? 0 : i_step) {
    ST *xrow = X + (size_t)id0 * F;
    if (!tile_ready) {  // first row of the wave, or the previous row ended before its last pass: plain row start
      cnt = ent_cnt;
      ent_col = opaque(ent_col);  // one wait for the staged entries, before the gathers (see fused_pass)
      ent_c = __int_as_float(opaque(__float_as_int(ent_c)));
      static_for<T / 8>([&](auto Pc) {
        constexpr int P = decltype(Pc)::value;
        if (8 * P < cnt) gather_pair<Tile, F, P>(y, cw, ent_col, ent_c, cnt, Y, lane);
      });
      slice(b1, e1, k0, ent_cnt);
      Tile::fetch(indices, data, opaque(lane), k0, max(k0 + ent_cnt, b1 + 1), ent_col, ent_c);
      if (leader) load_compact<F>(xrow, opaque(lane), x);  // last: loads complete in order and the row starts with x
      else kill(x);
    }
    // ent_* now describe row i + i_step
    float xc[FC], r[FC], p[FC], Ap[FC], rsold = 0.f;  // leader state
#pragma unroll
    for (int cc = 0; cc < FC; ++cc) xc[cc] = r[cc] = 0.f;
    bool store = false;
    if (leader) {
      put_operand(x);
#pragma unroll
      for (int cc = 0; cc < FC; ++cc) xc[cc] = x[cc];  // this row's iterate moves on as xc; x is re-loaded for the next row
      publish(kGo);
      if constexpr (TICKETS) {
        if (t3 < rows) draw();  // the ticket that follows t3; a team whose newest ticket is past the end draws no more
      }
    }
    unsigned w = await_operand();
    {
      float acc[FC];
      fused_pass<Tile, F, NJ, true, false, false>(y, cw, cnt, vt, j_begin, A0s, acc, lane, 0, ent_col, ent_c, Y, nullptr, nullptr, 0, 0);
      arrive(acc);
    }
    if (leader) {
      collect(r);
#pragma unroll
      for (int cc = 0; cc < FC; ++cc) r[cc] = -r[cc], p[cc] = r[cc];
      rsold = dot_compact<F>(r, r);
      store = rsold >= 1e-20f;  // else: x untouched (_als.pyx:206)
      if constexpr (TICKETS) {
        if (t3 < rows) take_draw();
      }
      if (store && cg_steps > 0) {
        put_operand(p);
        publish(kGo | (cg_steps == 1 ? kLast : 0u));
      } else {
        publish(stop_word());
      }
    }
    w = await_operand();
    for (int it = 0; (w & (kGo | kLast)) == kGo; ++it) {  // all steps but the last
      float acc[FC];
      fused_pass<Tile, F, NJ, false, false, false>(y, cw, cnt, vt, j_begin, A0s, acc, lane, 0, ent_col, ent_c, Y, nullptr, nullptr, 0, 0);
      arrive(acc);
      if (leader) {
        collect(Ap);
        get_operand(p);
        const float alpha = rsold * __builtin_amdgcn_rcpf(dot_compact<F>(p, Ap));
#pragma unroll
        for (int cc = 0; cc < FC; ++cc) {
          xc[cc] = fmaf(alpha, p[cc], xc[cc]);
          r[cc] = fmaf(-alpha, Ap[cc], r[cc]);
        }
        const float rsnew = dot_compact<F>(r, r);
        if (rsnew < 1e-20f) {
          publish(stop_word());  // the oracle breaks here (_als.pyx:235)
        } else {
          const float beta = rsnew * __builtin_amdgcn_rcpf(rsold);
#pragma unroll
          for (int cc = 0; cc < FC; ++cc) p[cc] = fmaf(beta, p[cc], r[cc]);
          rsold = rsnew;
          put_operand(p);
          publish(kGo | (it + 2 >= cg_steps ? kLast : 0u));
        }
      }
      w = await_operand();
    }
    // The last step stands outside the loop (the compiler must see that nothing of the row follows it): its pass rolls
    // the next row's tile in, and only its x update is evaluated -- the oracle's r, rsnew and p of the last step
    // (_als.pyx:226-241) are never read again, so neither is the vector A p: the pass hands back the wave's share of the
    // scalar p . A p (fused_pass, LAST) and the leader sums WPR floats.
    const bool rolled = Tile::ROLL && (w & kGo) != 0u;
    if (w & kGo) {
      float acc[FC], pAp;
      if constexpr (Tile::ROLL) {  // the tile of row i + i_step rolls in; the entries of row i + 2 i_step get staged
        int k2, cnt2;
        slice(b2, e2, k2, cnt2);
        if ((TICKETS ? t1 : i + i_step) >= rows) ent_cnt = 0;  // no next row (the schedule index is clamped): nothing to gather
        pAp = fused_pass<Tile, F, NJ, false, true, true>(y, cw, cnt, vt, j_begin, A0s, acc, lane, ent_cnt, ent_col, ent_c, Y, indices,
                                                         data, k2, max(k2 + cnt2, b2 + 1));
        cnt = ent_cnt;
        ent_cnt = cnt2;
        if (leader) load_compact<F>(X + (size_t)id1 * F, opaque(lane), x);  // the next row's iterate, into the carried registers
        else kill(x);
      } else {
        kill(x);
        pAp = fused_pass<Tile, F, NJ, false, true, false>(y, cw, cnt, vt, j_begin, A0s, acc, lane, 0, ent_col, ent_c, Y, nullptr,
                                                          nullptr, 0, 0);
      }
      arrive_scalar(pAp);
      if (leader) {
        pAp = collect_scalar(pAp);
        get_operand(p);
        const float alpha = rsold * __builtin_amdgcn_rcpf(pAp);
#pragma unroll
        for (int cc = 0; cc < FC; ++cc) xc[cc] = fmaf(alpha, p[cc], xc[cc]);
        publish(stop_word());
      }
      // the stop generation: keeps every wave's count in step with the leader's
      if constexpr (TICKETS) w = await_operand();
      else (void)await_operand();
    } else {
      kill(x);
    }
    if (leader && store) store_compact<F>(xrow, opaque(lane), xc);
    tile_ready = rolled;
    if constexpr (TICKETS) {
      // on every path `w` is now the row's stop word: the same ticket in every wavefront of the team
      i = t1, t1 = t2, t2 = t3, t3 = (int)(w >> 2);
      id0 = id1, id1 = id2, id2 = id3, id3 = row_id(t3);
    } else {
      id0 = id1, id1 = id2, id2 = id3, id3 = row_id(i + 4 * i_step);
    }
    b0 = b1, e0 = e1, b1 = b2, e1 = e2, b2 = indptr[id2], e2 = indptr[id2 + 1];
  }
}

}  // namespace imp
#endif  // IMPLICIT_AMD_CSRC_ALS_QF_COMMON_H_
