// K1h: float16 factor STORAGE with the tile kept as it is stored: the packed-half tile of the team kernel (als_qf_common.h)
// with als_cg_q64team_kernel -- round 4.
//
// Arithmetic contract: the oracle's CG (implicit/cpu/_als.pyx:152-248) in fp32 on the fp16-rounded factors, as the reference's
// kernels do for dtype = float16 (implicit/gpu/als.cu:41,55,109 + convert.cuh:7-17).
//
// The idea.  The resident-tile kernels are latency-bound pipelines: a team's rows advance one rendezvous per CG pass, a wavefront
// issues for ~13 % of that cycle, and what a SIMD retires is set by how many rows are in flight, i.e. by registers per row
// (DESIGN.md section 4.1).  The 32-entry fp32 tile (als_cg_qf.hip) converts an fp16 factor row at the load and holds it as fp32:
// half the HBM bytes, the same registers, no rolling gather through the conversion -- round 3 measured fp16 storage 8 % SLOWER
// than fp32.  Here a tile entry stays packed (two halves per register) for all passes and is widened inside the FMA
// (`v_fma_mix_f32`: f16 operand, fp32 accumulation; inline asm -- left to itself the compiler widens the tile once per pass and
// keeps the copy, 150 spilled registers), and the registers are spent on 64 entries per wavefront instead of 32: every row class
// runs on HALF the wavefronts (rows of 33..64 nonzeros on ONE, no team protocol at all; up to 128 on two, 256 on four, 512 on
// eight), twice the rows are in flight per CU, and the raw tile rolls in during the last pass again.
//
// What it buys, and what caps it.  configs[2], fp16 storage, per iteration (round 5, one box): row classes (32,64] / (64,128] /
// (128,256] / (256,512] 0.84 / 0.70 / 0.47 / 0.27 ms against 1.00 / 0.83 / 0.58 / 0.36 ms for the fp32-tile kernels (-18 %),
// whole iteration 4.39-4.53 against 4.91-4.96 ms -- fp16 storage is now level with fp32 storage (4.47-4.6 ms) instead of behind
// it.  It cannot get ahead: `v_fma_mix_f32` issues every 4.16 cycles per SIMD and `v_cvt_f32_f16` every 4.06, against 2.3 for a
// plain `v_fma_f32` and 4.4 for a `v_pk_fma_f32` that does TWO fp32 FMAs per lane (profiles/r04_micro_valu_rate.txt): widening a
// half costs as much issue time as the FMA it feeds, whichever instruction does it, so the tile part of a pass takes twice the
// vector time of the fp32 tile (round-5 timing-only knock-out builds, since removed: complete 4.70 ms, without the tile FMAs
// 4.03, without the gramian part 4.13, without both 3.23).  The only full-rate mixed form, `v_dot2c_f32_f16`, needs BOTH
// operands in f16.
#include <hip/hip_fp16.h>

#include "als_qf_common.h"
#include "common.h"

namespace imp {

namespace {
// d = float(half of yh) * b + c in ONE instruction.  Written as asm: given fmaf(half -> float, ..) twice on the same register (the
// dot and the axpy of an entry) the compiler converts the tile to fp32 once per pass and keeps the copy -- 64 more live registers,
// i.e. the very thing the packed tile exists to avoid (150 spilled registers).
__device__ __forceinline__ float fma_mix_lo(unsigned yh, float b, float c) {
  float d;
  asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(d) : "v"(yh), "v"(b), "v"(c));
  return d;
}
__device__ __forceinline__ float fma_mix_hi(unsigned yh, float b, float c) {
  float d;
  asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(yh), "v"(b), "v"(c));
  return d;
}
__device__ __forceinline__ float mul_mix_lo(unsigned yh, float b) {
  float d;
  asm("v_fma_mix_f32 %0, %1, %2, 0 op_sel_hi:[1,0,0]" : "=v"(d) : "v"(yh), "v"(b));
  return d;
}
__device__ __forceinline__ float mul_mix_hi(unsigned yh, float b) {
  float d;
  asm("v_fma_mix_f32 %0, %1, %2, 0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(yh), "v"(b));
  return d;
}

// The packed-half tile: 64 entries per wavefront, 16 per 16-lane group; one register holds expanded slots (2 h, 2 h + 1) of an
// entry as two halves, so the tile takes the registers of the 32-entry fp32 tile.  (The fp32 form of this tile -- a packed fp32
// pair per element, two "fat" wavefronts per SIMD -- measured slower than the 32-entry tiles in round 4 and was removed in
// round 6.)
struct Tile64 {
  typedef unsigned elem;
  static constexpr int T = 64;
  static constexpr bool ROLL = true;
  // entry t of the slice in lane t: all 64 lanes
  static __device__ __forceinline__ void fetch(const int32_t *__restrict__ indices, const float *__restrict__ data, int lane, int k0,
                                               int end, int &col, float &c) {
    const int k = min(k0 + lane, end - 1);
    col = indices[k];
    c = data[k];
  }
  template <int H> static __device__ __forceinline__ void gather(elem (&yq)[H], const __half *p) {
#pragma unroll
    for (int h = 0; h < H; h += 2) {  // 4 halves = one 8-byte load
      const uint2 raw = *reinterpret_cast<const uint2 *>(p + 32 * h);
      yq[h] = raw.x, yq[h + 1] = raw.y;
    }
  }
  template <int H> static __device__ __forceinline__ float dot(const elem (&yq)[H], const f32x2 (&ve)[H]) {
    float s0 = mul_mix_lo(yq[0], ve[0].x), s1 = mul_mix_hi(yq[0], ve[0].y);
#pragma unroll
    for (int h = 1; h < H; ++h) {
      s0 = fma_mix_lo(yq[h], ve[h].x, s0);
      s1 = fma_mix_hi(yq[h], ve[h].y, s1);
    }
    return s0 + s1;
  }
  template <int H> static __device__ __forceinline__ void axpy(const elem (&yq)[H], float w, f32x2 (&ae)[H]) {
#pragma unroll
    for (int h = 0; h < H; ++h) {
      ae[h].x = fma_mix_lo(yq[h], w, ae[h].x);
      ae[h].y = fma_mix_hi(yq[h], w, ae[h].y);
    }
  }
};
}  // namespace

template <int F, int WPR, int BLOCK, typename ST>
__global__ __launch_bounds__(BLOCK, F == 64 ? 8 : 4) void als_cg_q64team_kernel(
    const int32_t *__restrict__ order, int first, int count, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
    const float *__restrict__ data, ST *__restrict__ X, const ST *__restrict__ Y, const float *__restrict__ A0, int cg_steps) {
  team_rows<Tile64, F, WPR, BLOCK>(order, first, count, indptr, indices, data, X, Y, A0, cg_steps);
}

template <int F, int WPR, int BLOCK, typename ST>
static void launch_q64team(const imp_csr *C, int first, int count, ST *X, const ST *Y, const float *A0, int cg_steps, const char *name) {
  if (count <= 0) return;
  constexpr int WAVES = BLOCK / 64, TEAMS = WAVES / WPR;
  const size_t lds = team_lds_bytes<F, WPR, BLOCK, Tile64::T>();
  auto kern = als_cg_q64team_kernel<F, WPR, BLOCK, ST>;
  allow_dynamic_lds(kern, lds);
  int per_cu = 0;  // workgroups per CU as the registers and the LDS allow
  IMP_CHECK_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, BLOCK, lds));
  per_cu = std::max(1, per_cu);
  constexpr int kBaseOversub = WPR <= 2 ? 4 : 2;  // as launch_qfteam for the same row classes
  const int grid = std::min((count + TEAMS - 1) / TEAMS, ctx().num_cus * per_cu * std::max(kBaseOversub, ctx().oversub));
  IMP_PROF(name);
  kern<<<grid, BLOCK, lds, stream()>>>(C->order.data(), first, count, C->indptr.data(), C->indices.data(), C->data.data(), X, Y, A0,
                                      cg_steps);
  IMP_CHECK_HIP(hipGetLastError());
}

// width: wavefronts per row, 1 / 2 / 4 / 8 (rows of up to 64 / 128 / 256 / 512 nonzeros)
template <typename ST>
void launch_team_tile64(const imp_csr *C, int f, int width, int first, int count, ST *X, const ST *Y, const float *A0, int cg_steps,
                        const char *name) {
  auto run = [&](auto Fc) {
    constexpr int F = decltype(Fc)::value;
    switch (width) {
      case 8: launch_q64team<F, 8, 512, ST>(C, first, count, X, Y, A0, cg_steps, name); break;
      case 4: launch_q64team<F, 4, 512, ST>(C, first, count, X, Y, A0, cg_steps, name); break;
      case 2: launch_q64team<F, 2, 512, ST>(C, first, count, X, Y, A0, cg_steps, name); break;
      case 1: launch_q64team<F, 1, 512, ST>(C, first, count, X, Y, A0, cg_steps, name); break;
      default: throw std::invalid_argument("launch_team_tile64: team width");
    }
  };
  if (f == 128) run(idx_t<128>{});
  else if (f == 64) run(idx_t<64>{});
  else throw std::invalid_argument("launch_team_tile64: f must be 64 or 128");
}
template void launch_team_tile64<__half>(const imp_csr *, int, int, int, int, __half *, const __half *, const float *, int, const char *);

}  // namespace imp
