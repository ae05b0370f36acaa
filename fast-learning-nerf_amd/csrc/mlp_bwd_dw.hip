// mlp_bwd_dw.hip -- dW = dY^T X per layer (+ bias column sums, + the alpha head's rank-1 row), the head gradients, the ordered reduction of the
// per-workgroup partials, and the backward entry points (which launch the dX kernel of mlp_bwd_dx.hip first).
#include "mlp_common.h"
#include "dw_pair.h"
#include <atomic>

int fn_launch_dx(int mm, int grid, hipStream_t st, int64_t P, const float* draw, const float* act, const float* params, const float* packed_bwd,
                 float* dact, const NetLayout& L, const int* live_idx, const int* live_cnt, float* headws, int flags);   // mlp_bwd_dx.hip

// =========================================================================================
// backward: dW = dY^T X  (split over workgroups by point chunk, partials reduced afterwards)
// =========================================================================================
#define DW_MT 32  // points per LDS stage

// WO x WI waves (4 or 8), each wave TO x TI MFMA tiles:  NO = WO*TO*32, KI = WI*TI*32.
// The 256x256 jobs run 8 waves x 128 accumulator registers (two waves per SIMD) so that one wave's
// staging / bias work overlaps the other's MFMAs.
template <int WO, int WI, int TO, int TI, bool BIAS, bool RANK1>     // (the fp32-MFMA dW; bf16x6: mlp_bwd_dw6_kernel below)
__global__ void __launch_bounds__(WO * WI * 64, WO * WI / 4)
mlp_bwd_dw_kernel(int64_t P, const float* __restrict__ dY, int ldy, const float* __restrict__ X, int ldx,
                  const float* __restrict__ draw /*RANK1: dalpha = draw[p*4+3]*/, float* __restrict__ partial_w,
                  float* __restrict__ partial_b, float* __restrict__ partial_r, const int* __restrict__ live_idx,
                  const int* __restrict__ live_cnt) {
  if (live_idx) P = (int64_t)__builtin_amdgcn_readfirstlane(*live_cnt);   // live-list mode: rows 0 .. *live_cnt of dY / X
  constexpr int NO = WO * TO * 32, KI = WI * TI * 32;
  constexpr int NTD = WO * WI * 64;  // threads
  constexpr int STAGE = DW_MT * (NO + KI) + DW_MT;  // floats per LDS stage (+32 dalpha)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wo = wave / WI, wi = wave % WI;
  // contiguous chunk of points for this workgroup (multiple of DW_MT)
  const int64_t ntile_all = (P + DW_MT - 1) / DW_MT;
  const int64_t per = (ntile_all + gridDim.x - 1) / gridDim.x;
  const int64_t t0 = blockIdx.x * per;
  int64_t t1 = t0 + per;
  if (t1 > ntile_all) t1 = ntile_all;

  f32x16 acc[TO][TI];
#pragma unroll
  for (int a = 0; a < TO; ++a)
#pragma unroll
    for (int b = 0; b < TI; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
  float bsum = 0.f, rsum = 0.f;

  constexpr int YV = (DW_MT * NO / 4 + NTD - 1) / NTD;  // float4 per thread for the dY stage
  constexpr int XV = (DW_MT * KI / 4 + NTD - 1) / NTD;  // float4 per thread for the X stage
  static_assert(DW_MT * NO % 4 == 0 && DW_MT * KI % 4 == 0 && NO <= NTD && KI <= NTD, "stage split");
  float4 ry[YV], rx[XV];
  float rda = 0.f;

  auto load_stage = [&](int64_t t) {
    const int64_t pbase = t * DW_MT;
#pragma unroll
    for (int i = 0; i < YV; ++i) {
      const int e = (i * NTD + tid) * 4;
      const int m = e / NO, c = e % NO;
      const int64_t p = pbase + m;
      ry[i] = (e < DW_MT * NO && p < P) ? *reinterpret_cast<const float4*>(dY + p * ldy + c)
                                        : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int i = 0; i < XV; ++i) {
      const int e = (i * NTD + tid) * 4;
      const int m = e / KI, c = e % KI;
      const int64_t p = pbase + m;
      rx[i] = (e < DW_MT * KI && p < P) ? *reinterpret_cast<const float4*>(X + p * ldx + c)
                                        : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (RANK1 && tid < DW_MT) {
      const int64_t p = pbase + tid;
      rda = (p < P) ? draw[(live_idx ? (int64_t)live_idx[p] : p) * 4 + 3] : 0.f;
    }
  };
  auto store_stage = [&](float* st) {
#pragma unroll
    for (int i = 0; i < YV; ++i)
      if ((i * NTD + tid) * 4 < DW_MT * NO) *reinterpret_cast<float4*>(st + (i * NTD + tid) * 4) = ry[i];
#pragma unroll
    for (int i = 0; i < XV; ++i)
      if ((i * NTD + tid) * 4 < DW_MT * KI) *reinterpret_cast<float4*>(st + DW_MT * NO + (i * NTD + tid) * 4) = rx[i];
    if (RANK1 && tid < DW_MT) st[DW_MT * (NO + KI) + tid] = rda;
  };

  if (t0 < t1) {
    load_stage(t0);
    store_stage(smem);
  }
  __syncthreads();
  for (int64_t t = t0; t < t1; ++t) {
    float* cur = smem + ((t - t0) & 1) * STAGE;
    float* nxt = smem + (((t - t0) & 1) ^ 1) * STAGE;
    if (t + 1 < t1) load_stage(t + 1);
    const float* Ys = cur;
    const float* Xs = cur + DW_MT * NO;
    // MFMA over the stage's 32 points, 2 per step; fragments of the next step are fetched from LDS
    // before the current step's MFMAs are issued (ping-pong registers): with one wave per SIMD
    // nothing else hides the ds_read latency.
    {
      float fa0[TO], fb0[TI], fa1[TO], fb1[TI];
      auto ldf = [&](float (&a)[TO], float (&b)[TI], int k2) {
        const int m = k2 * 2 + (lane >> 5);
#pragma unroll
        for (int i = 0; i < TO; ++i) a[i] = Ys[m * NO + (wo * TO + i) * 32 + (lane & 31)];
#pragma unroll
        for (int j = 0; j < TI; ++j) b[j] = Xs[m * KI + (wi * TI + j) * 32 + (lane & 31)];
      };
      auto mm = [&](const float (&a)[TO], const float (&b)[TI]) {
#pragma unroll
        for (int i = 0; i < TO; ++i)
#pragma unroll
          for (int j = 0; j < TI; ++j) acc[i][j] = mfma(a[i], b[j], acc[i][j]);
      };
      ldf(fa0, fb0, 0);
#pragma unroll
      for (int k2 = 0; k2 < DW_MT / 2; k2 += 2) {
        // sched_barrier: keep the LDS reads AHEAD of the MFMA block (the machine scheduler otherwise
        // sinks them next to their first use and re-exposes the latency)
        ldf(fa1, fb1, k2 + 1);
        __builtin_amdgcn_sched_barrier(0);
        mm(fa0, fb0);
        __builtin_amdgcn_sched_barrier(0);
        if (k2 + 2 < DW_MT / 2) ldf(fa0, fb0, k2 + 2);
        __builtin_amdgcn_sched_barrier(0);
        mm(fa1, fb1);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (BIAS) {
      if (tid < NO) {
#pragma unroll 8
        for (int m = 0; m < DW_MT; ++m) bsum += Ys[m * NO + tid];
      }
    }
    if (RANK1) {
      if (tid < KI) {
        const float* da = cur + DW_MT * (NO + KI);
#pragma unroll 8
        for (int m = 0; m < DW_MT; ++m) rsum = fmaf(da[m], Xs[m * KI + tid], rsum);
      }
    }
    if (t + 1 < t1) store_stage(nxt);
    __syncthreads();
  }
  // write partials
  float* pw = partial_w + (int64_t)blockIdx.x * NO * KI;
#pragma unroll
  for (int i = 0; i < TO; ++i)
#pragma unroll
    for (int j = 0; j < TI; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int o = (wo * TO + i) * 32 + crow(r, lane);
        const int c = (wi * TI + j) * 32 + (lane & 31);
        pw[(int64_t)o * KI + c] = acc[i][j][r];
      }
  if (BIAS && tid < NO) partial_b[(int64_t)blockIdx.x * NO + tid] = bsum;
  if (RANK1 && tid < KI) partial_r[(int64_t)blockIdx.x * KI + tid] = rsum;
}

// ---------------------------------------------------------------------------------------------------------------------
// MM_X6 dW.  On this chip a SIMD issues NOTHING VALU-class while one of its waves streams v_mfma_f32_32x32x16_bf16 back to back
// (tools/micro/coexec_split.hip, profiles/r03_mfma_valu_exclusion.md): the partner wave's VALU work does not hide under the MFMAs,
// it adds to them; only LDS / memory latency overlaps.  The synchronous stage of mlp_bwd_dw_kernel (global -> registers -> fp32 LDS
// -> barrier, then every wave gathers and splits the fragments it multiplies) split every dY tile in the WI waves that share it
// and every X tile in WO waves -- three quarters of that arithmetic was redundant, and all of it was serial with the MFMAs
// (51 % matrix-pipe busy; 66 % with this kernel, profiles/r03_sq_counters.md).  Here
//   * a k-step is 16 points; its (NO + KI) / 32 operand tiles are split ONCE, each by one wave: a lane loads its 8 consecutive
//     points of a channel straight from global memory (32 lanes = one 128-byte line per point) into registers TWO k-steps ahead
//     (counted vmcnt waits: no control flow between a load and its use), splits them (split3_frag) and stores the three bf16
//     pieces as fragment-ordered 1 KiB planes into the split buffer S; the bias column sums / the rank-1 row come from the same
//     registers;
//   * S is double-buffered (2 x 48 KiB for the 256 x 256 jobs): k-step q + 1 is split after k-step q has been multiplied, ONE
//     barrier per k-step; a wave's MFMA operands are three ds_read_b128 per tile;
//   * whole k-steps address with a wave-uniform base + immediates (no per-lane address arithmetic); the k-steps that touch the
//     end of the workgroup's row range clamp their rows and zero them when they are split.
// ---------------------------------------------------------------------------------------------------------------------
// CTI2 > 0: the last CTI2 of the WI * TI input tiles come from a second tensor X2 of width 32 * CTI2 (the view layer's two inputs,
// feature and encoded direction, ride in ONE job: their common dY is read and split once).
// CTO2 > 0: the last CTO2 of the WO * TO output tiles come from a second gradient tensor dY2 of width 32 * CTO2 (layers 0 and 5 both
// multiply the positional encoding: it is read and split once); bias sums are taken over dY only.
// wg / nwg: this workgroup's chunk of the k-steps and the number of chunks (mlp_bwd_dw6_kernel: blockIdx.x / gridDim.x; the trunk
// launch below: blockIdx.x / a function of the point count)
// RBV (the view job, no live list): the dY tiles are REBUILT in the splitting lane instead of read -- dYv = (drgb . Wr) [hv > 0], dX's own expression
// (dyv_value, mlp_common.h: bit-identical to what dX stores).  `dY` points at hv (same shape as dYv), wave 0 stages draw as a whole float4 (DR
// beside DA, the same lanes, the same loads one pair of k-steps ahead) and a lane keeps the three Wr values of its channel; dYv is neither
// written (dX) nor read.  Bias column sums are taken over the rebuilt values.
template <int WO, int WI, int TO, int TI, bool BIAS, bool RANK1, int CTI2 = 0, int CTO2 = 0, bool RBV = false>
__device__ __forceinline__ void dw6_body(const int64_t P, const float* __restrict__ dY, const float* __restrict__ X,
                                         const float* __restrict__ draw, float* __restrict__ partial_w, float* __restrict__ partial_b,
                                         float* __restrict__ partial_r, const int* __restrict__ live_idx,
                                         const float* __restrict__ X2, const float* __restrict__ dY2, const int wg, const int nwg,
                                         const float* __restrict__ rb_wr = nullptr) {
  constexpr int NO = WO * TO * 32, KI = WI * TI * 32;
  constexpr int CTO = WO * TO, CTI = WI * TI, NTILE = CTO + CTI;
  constexpr int NW = WO * WI;
  constexpr int TPW = (NTILE + NW - 1) / NW;         // tiles a wave splits per k-step
  extern __shared__ __attribute__((aligned(16))) uint4 S6[];   // [2][tile][piece h | m | l][lane]
  float* const DA = reinterpret_cast<float*>(S6 + 2 * NTILE * 192);   // RANK1: dalpha of the 16 points of a k-step, [2][16]
  float4* const DR = reinterpret_cast<float4*>(DA + 32);              // RBV: draw of the 16 points of a k-step, [2][16]
  static_assert(!RBV || (RANK1 && CTO2 == 0), "the view job: draw is staged, one gradient tensor");
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wo = wave / WI, wi = wave % WI;
  const int64_t nq_all = (P + 15) / 16;
  const int64_t per = (nq_all + nwg - 1) / nwg;
  const int64_t q0 = wg * per;
  int64_t q1 = q0 + per;
  if (q1 > nq_all) q1 = nq_all;
  const int nq = (int)(q1 - q0);
  int64_t Pend = q1 * 16;                             // rows this workgroup may read
  if (Pend > P) Pend = P;

  f32x16 acc[TO][TI];
#pragma unroll
  for (int a = 0; a < TO; ++a)
#pragma unroll
    for (int b = 0; b < TI; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
  float ssum[TPW];   // side sums of the tiles THIS wave splits: bias column sums (dY tiles) / rank-1 row (X tiles)
#pragma unroll
  for (int k = 0; k < TPW; ++k) ssum[k] = 0.f;

  // the tiles this wave splits: tile t = k * NW + wave; t < CTO: channels t*32.. of dY, else channels (t - CTO)*32.. of X.
  // Rows are counted from the workgroup's first row.
  constexpr int CTI1 = CTI - CTI2, KI1 = CTI1 * 32, KI2 = CTI2 * 32;   // row widths of X and X2 (KI = KI1 + KI2 partial columns)
  // (RANK1 with CTI2: the rank-1 row is taken over X only, KI1 columns -- the folded view job: X = h7, X2 = the encoded direction)
  constexpr int CTO1 = CTO - CTO2, NO1 = CTO1 * 32, NO2 = CTO2 * 32;   // row widths of dY and dY2 (NO = NO1 + NO2 partial rows)
  static_assert(!(RANK1 && CTO2) && !(CTI2 && CTO2), "one second tensor per job");
  const float* tsrc[TPW];
  bool tisy[TPW], tis2[TPW];   // tis2: the tile comes from the second tensor of its side
  // KNOWN: the wave count divides the number of dY tiles and there is no second tensor (the 256 x 256 jobs: 14 of a step's 22 launches):
  // whether slot k holds a dY or an X tile is then the same for every wave and known at compile time -- no wave-uniform branch splits the
  // main loop's body, which is what lets the split of k-step q + 1 be scheduled between the MFMAs of k-step q (X6_DW_PIPE below)
  constexpr bool KNOWN = (CTO % NW == 0) && (NTILE % NW == 0) && CTO2 == 0 && CTI2 == 0;
#pragma unroll
  for (int k = 0; k < TPW; ++k) {
    const int t = k * NW + wave;
    tisy[k] = KNOWN ? (k * NW < CTO) : (t < CTO);
    tis2[k] = (CTI2 > 0 && t >= CTO + CTI1) || (CTO2 > 0 && t >= CTO1 && t < CTO);
    tsrc[k] = tisy[k] ? (tis2[k] ? dY2 + q0 * (16 * NO2) + (t - CTO1) * 32 : dY + q0 * (16 * NO1) + t * 32)
                      : (tis2[k] ? X2 + q0 * (16 * KI2) + (t - CTO - CTI1) * 32 : X + q0 * (16 * KI1) + (t - CTO) * 32);
  }
  const int relmax = (int)(Pend - q0 * 16) - 1;   // last row of this workgroup (nq > 0: >= 0)
  const int col = lane & 31, half8 = (lane >> 5) * 8;
  const unsigned boffy = (unsigned)(half8 * NO1 + col) * 4u, boffy2 = (unsigned)(half8 * NO2 + col) * 4u,
                 boffx = (unsigned)(half8 * KI1 + col) * 4u, boffx2 = (unsigned)(half8 * KI2 + col) * 4u;   // byte offsets of row 0
  struct Raw { float v[TPW][8]; };
  float wr0[TPW], wr1[TPW], wr2[TPW];   // RBV: the Wr column of the lane's dYv channel, per slot
  if constexpr (RBV) {
#pragma unroll
    for (int k = 0; k < TPW; ++k) {
      const int t = k * NW + wave;
      if (tisy[k] && (NTILE % NW == 0 || t < NTILE)) {
        wr0[k] = rb_wr[t * 32 + col]; wr1[k] = rb_wr[128 + t * 32 + col]; wr2[k] = rb_wr[256 + t * 32 + col];
      } else {
        wr0[k] = wr1[k] = wr2[k] = 0.f;
      }
    }
  }
  auto ldb = [](const float* base, unsigned byte_off) __attribute__((always_inline)) -> float {   // uniform base + 32-bit offset
    return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + byte_off);
  };
  // whole = std::true_type: every row of the k-step exists (straight-line code, counted waits); false_type: rows beyond the range
  // are clamped to the last row here and zeroed in split_store (the last k-steps of a workgroup, and the two-ahead loads past them)
  auto load_raw = [&](Raw& r, int st, auto whole) __attribute__((always_inline)) {   // st = k-step of this workgroup
    if constexpr (decltype(whole)::value) {
#pragma unroll
      for (int k = 0; k < TPW; ++k) {
        const int t = k * NW + wave;
        if (NTILE % NW == 0 || t < NTILE) {
          if (tisy[k] && CTO2 > 0 && tis2[k]) {
            const float* b = tsrc[k] + (int64_t)st * (16 * NO2);
#pragma unroll
            for (int e = 0; e < 8; ++e) r.v[k][e] = ldb(b, boffy2 + (unsigned)(e * NO2 * 4));
          } else if (tisy[k]) {
            const float* b = tsrc[k] + (int64_t)st * (16 * NO1);
#pragma unroll
            for (int e = 0; e < 8; ++e) r.v[k][e] = ldb(b, boffy + (unsigned)(e * NO1 * 4));
          } else if (CTI2 > 0 && tis2[k]) {
            const float* b = tsrc[k] + (int64_t)st * (16 * KI2);
#pragma unroll
            for (int e = 0; e < 8; ++e) r.v[k][e] = ldb(b, boffx2 + (unsigned)(e * KI2 * 4));
          } else {
            const float* b = tsrc[k] + (int64_t)st * (16 * KI1);
#pragma unroll
            for (int e = 0; e < 8; ++e) r.v[k][e] = ldb(b, boffx + (unsigned)(e * KI1 * 4));
          }
        }
      }
    } else {
      unsigned row[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) { const int rr = st * 16 + half8 + e; row[e] = (unsigned)(rr < relmax ? rr : relmax); }
#pragma unroll
      for (int k = 0; k < TPW; ++k) {
        const int t = k * NW + wave;
        if (NTILE % NW == 0 || t < NTILE) {
#pragma unroll
          for (int e = 0; e < 8; ++e)
            r.v[k][e] = ldb(tsrc[k], (row[e] * (unsigned)(tisy[k] ? (tis2[k] ? NO2 : NO1) : (tis2[k] ? KI2 : KI1)) + (unsigned)col) * 4u);
        }
      }
    }
  };
  // RANK1: d(loss)/d(sigma) = draw[p][3], one point per lane 0..15 of wave 0, staged through LDS one k-step ahead of the split that
  // multiplies it.  Two dependent loads in live mode (row -> point -> draw), each issued one pair of k-steps ahead of its use.
  const int* const li = live_idx ? live_idx : reinterpret_cast<const int*>(draw);   // (a valid address when there is no list)
  auto load_ix = [&](int st) __attribute__((always_inline)) -> int64_t {
    const int rr = st * 16 + (lane & 15);
    const int64_t p = q0 * 16 + (rr < relmax ? rr : relmax);
    const int64_t lv = li[p];
    return live_idx ? lv : p;
  };
  auto split_store = [&](const Raw& r, int buf, int st, auto whole) __attribute__((always_inline)) {
    const int nv = relmax + 1 - (st * 16 + half8);         // this lane's rows e < nv exist
#pragma unroll
    for (int k = 0; k < TPW; ++k) {
      const int t = k * NW + wave;
      if (NTILE % NW == 0 || t < NTILE) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = r.v[k][e];
        if constexpr (RBV) {
          if (tisy[k]) {   // r holds hv
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float4 d = DR[(st & 1) * 16 + half8 + e];
              v[e] = dyv_value(v[e], d.x, d.y, d.z, wr0[k], wr1[k], wr2[k]);
            }
          }
        }
        if constexpr (!decltype(whole)::value) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = e < nv ? v[e] : 0.f;
        }
        uint4 h, m, l;
        uint4* d = S6 + ((buf * NTILE + t) * 3) * 64 + lane;
        split3_frag(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), h, m, l);
        d[0] = h; d[64] = m; d[128] = l;
        if (BIAS && (KNOWN ? (k * NW < CTO) : (t < CTO1))) ssum[k] += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
        if (RANK1 && (KNOWN ? (k * NW >= CTO) : (t >= CTO && t < CTO + CTI1))) {
          const float4 d0 = *reinterpret_cast<const float4*>(DA + (st & 1) * 16 + half8);
          const float4 d1 = *reinterpret_cast<const float4*>(DA + (st & 1) * 16 + half8 + 4);
          const float da[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
#pragma unroll
          for (int e = 0; e < 8; ++e) ssum[k] = fmaf(da[e], v[e], ssum[k]);
        }
      }
    }
  };
  // six-product MFMAs of the k-step held by S[buf]; X tiles two at a time, product-major over the 2 x TO accumulators of the
  // pair: consecutive MFMAs never target the same accumulator (a dependent MFMA waits for its predecessor's full latency)
  auto multiply = [&](int buf) __attribute__((always_inline)) {
    const uint4* Sb = S6 + buf * NTILE * 192 + lane;
    uint4 a[TO][3];
#pragma unroll
    for (int i = 0; i < TO; ++i)
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) a[i][pl] = Sb[((wo * TO + i) * 3 + pl) * 64];
    constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};   // small terms first
    constexpr int JP = TI >= 2 ? 2 : 1;
#pragma unroll
    for (int j0 = 0; j0 < TI; j0 += JP) {
      uint4 b[JP][3];
#pragma unroll
      for (int jj = 0; jj < JP; ++jj)
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
          if (j0 + jj < TI) b[jj][pl] = Sb[((CTO + wi * TI + j0 + jj) * 3 + pl) * 64];
#pragma unroll
      for (int t = 0; t < 6; ++t)
#pragma unroll
        for (int jj = 0; jj < JP; ++jj)
#pragma unroll
          for (int i = 0; i < TO; ++i)
            if (j0 + jj < TI) acc[i][j0 + jj] = mfma_bf16(a[i][PA[t]], b[jj][PB[t]], acc[i][j0 + jj]);
    }
  };
  auto publish = [&]() __attribute__((always_inline)) {   // S pieces written / fragments read: hand the buffers over
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  };

  if (nq > 0) {
    // k-steps in pairs (S[0] / registers r0 hold the even ones); a trailing odd k-step multiplies a stage of zeros
    constexpr std::true_type WHOLE{};
    constexpr std::false_type ANY{};
    Raw r0, r1;
    load_raw(r0, 0, ANY);
    load_raw(r1, 1, ANY);
    // RANK1, wave 0, lanes 0..15: dalpha of the k-steps 2, 4, ... / 3, 5, ... on their way to DA, and the points after them
    // (RBV: the whole float4 -- .w to DA as before, all of it to DR for the lanes that rebuild dYv)
    typedef typename std::conditional<RBV, float4, float>::type DrawT;
    auto ld_draw = [&](int64_t ix) __attribute__((always_inline)) -> DrawT {
      if constexpr (RBV) return *reinterpret_cast<const float4*>(draw + ix * 4);
      else return draw[ix * 4 + 3];
    };
    auto st_draw = [&](int slot, const DrawT& d) __attribute__((always_inline)) {
      if constexpr (RBV) { DA[slot] = d.w; DR[slot] = d; }
      else DA[slot] = d;
    };
    DrawT dr0 = DrawT(), dr1 = DrawT();
    int64_t ix0 = 0, ix1 = 0;
    const bool da_lane = RANK1 && wave == 0 && lane < 16;
    if (da_lane) {
      st_draw(lane, ld_draw(load_ix(0)));
      st_draw(16 + lane, ld_draw(load_ix(1)));
      dr0 = ld_draw(load_ix(2));
      dr1 = ld_draw(load_ix(3));
      ix0 = load_ix(4);
      ix1 = load_ix(5);
    }
    if (RANK1) publish();
    split_store(r0, 0, 0, ANY);
    load_raw(r0, 2, ANY);
    publish();
    auto mix = [&](auto sync) __attribute__((always_inline)) {   // (one pipeline per half of the loop body: distinct sync ids)
      if constexpr (KNOWN && !RANK1) interleave6<0, TO * TI * 6, TPW * 4 * 11 + (BIAS ? 8 : 0), decltype(sync)::value>();
    };
    auto pair = [&](int d, auto whole) __attribute__((always_inline)) {
      const int st = 2 * d;
      if (da_lane) { st_draw(lane, dr0); dr0 = ld_draw(ix0); ix0 = load_ix(st + 6); }
      multiply(0);
      split_store(r1, 1, st + 1, whole);
      mix(std::integral_constant<int, 1>{});
      load_raw(r1, st + 3, whole);
      publish();
      if (da_lane) { st_draw(16 + lane, dr1); dr1 = ld_draw(ix1); ix1 = load_ix(st + 7); }
      multiply(1);
      split_store(r0, 0, st + 2, whole);
      mix(std::integral_constant<int, 2>{});
      load_raw(r0, st + 4, whole);
      publish();
    };
    const int n2 = (nq + 1) / 2;
    const int nwhole = (relmax + 1) / 16;                     // k-steps 0 .. nwhole - 1 have all their rows
    int dmain = nwhole >= 5 ? (nwhole - 3) / 2 : 0;           // pairs whose k-steps up to 2 d + 4 are whole
    if (dmain > n2) dmain = n2;
#pragma unroll 1
    for (int d = 0; d < dmain; ++d) pair(d, WHOLE);
#pragma unroll 1
    for (int d = dmain; d < n2; ++d) pair(d, ANY);
  }
  // write partials (zeros from workgroups without points: reduce_all sums every chunk's region)
  float* pw = partial_w + (int64_t)wg * NO * KI;
#pragma unroll
  for (int i = 0; i < TO; ++i)
#pragma unroll
    for (int j = 0; j < TI; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int o = (wo * TO + i) * 32 + crow(r, lane);
        const int c = (wi * TI + j) * 32 + (lane & 31);
        pw[(int64_t)o * KI + c] = acc[i][j][r];
      }
  if (BIAS || RANK1) {
#pragma unroll
    for (int k = 0; k < TPW; ++k) {
      const int t = k * NW + wave;
      if (NTILE % NW == 0 || t < NTILE) {
        const float sv = ssum[k] + __shfl_xor(ssum[k], 32, 64);
        if (lane < 32) {
          if (BIAS && t < CTO1) partial_b[(int64_t)wg * NO1 + t * 32 + lane] = sv;
          if (RANK1 && t >= CTO && t < CTO + CTI1) partial_r[(int64_t)wg * KI1 + (t - CTO) * 32 + lane] = sv;
        }
      }
    }
  }
}

template <int WO, int WI, int TO, int TI, bool BIAS, bool RANK1, int CTI2 = 0, int CTO2 = 0>
__global__ void __launch_bounds__(WO * WI * 64, WO * WI / 4)
mlp_bwd_dw6_kernel(int64_t P, const float* __restrict__ dY, const float* __restrict__ X,
                   const float* __restrict__ draw, float* __restrict__ partial_w, float* __restrict__ partial_b,
                   float* __restrict__ partial_r, const int* __restrict__ live_idx, const int* __restrict__ live_cnt,
                   const float* __restrict__ X2 = nullptr, const float* __restrict__ dY2 = nullptr) {
  if (live_idx) P = (int64_t)__builtin_amdgcn_readfirstlane(*live_cnt);
  dw6_body<WO, WI, TO, TI, BIAS, RANK1, CTI2, CTO2>(P, dY, X, draw, partial_w, partial_b, partial_r, live_idx, X2, dY2, (int)blockIdx.x,
                                                    (int)gridDim.x);
}

// the rebuilding view job (dw6_body RBV): hv where dYv was, Wr of the net
template <int WO, int WI, int TO, int TI, bool BIAS, bool RANK1, int CTI2>
__global__ void __launch_bounds__(WO * WI * 64, WO * WI / 4)
mlp_bwd_dw6_rbv_kernel(int64_t P, const float* __restrict__ hv, const float* __restrict__ X, const float* __restrict__ draw,
                       float* __restrict__ partial_w, float* __restrict__ partial_b, float* __restrict__ partial_r,
                       const float* __restrict__ X2, const float* __restrict__ wr) {
  dw6_body<WO, WI, TO, TI, BIAS, RANK1, CTI2, 0, true>(P, hv, X, draw, partial_w, partial_b, partial_r, nullptr, X2, nullptr, (int)blockIdx.x,
                                                       (int)gridDim.x, wr);
}

// ---------------------------------------------------------------------------------------------------------------------
// The seven 256 x 256 jobs of a pass (L1 .. L7; the feature layer's job is gone with the fold, its rank-1 row rides the view job) in ONE launch:
// grid = (chunks, 7 jobs).  The number of split-K chunks per job is a function of the POINT COUNT ALONE (dw_trunk_chunks: an eighth of the chip per
// 256 k-steps of 16 points, between 1/8 of the CUs and all of them), so that
//   * the partials and their reduction shrink with the batch: a 512-ray shard (the reference's configs train at 1024 - 1920 rays,
//     lego.txt:16; an 8-way strong-scaling shard of BASELINE configs[1] is 512) writes 32 chunks per job instead of 256 -- 75 MB per
//     pass through reduce_all instead of 0.7 GB -- while 8 jobs x ncu / 8 chunks still fill every CU with whole rounds of equal work;
//   * the order in which partial sums meet depends on the point count only: the live-list backward (device-side count) chunks exactly like
//     the plain backward of the same points -- bit-identical gradients (tests/test_gpu_compact.py).  The host sizes the grid for
//     the capacity P_total; chunks beyond dw_trunk_chunks(P) exit and are not reduced.
// The host checks dw_trunk_chunks(P) <= the chunks a partial region holds before every trunk launch (trunk_chunks_fit).  When one call runs
// both passes of a two-net step, their 14 jobs go into ONE launch with the same chunking: mlp_bwd_dw6_trunk_pair_kernel below.
// ---------------------------------------------------------------------------------------------------------------------
#define DW_QMAX 256   // k-steps (of 16 points) a chunk grows to before the next eighth of the chip is added
__host__ __device__ static inline int dw_trunk_chunks(int64_t P, int ncu) {
  const int unit = ncu >= 8 ? ncu / 8 : 1;
  const int64_t nq = (P + 15) / 16;
  int64_t k = (nq + (int64_t)unit * DW_QMAX - 1) / ((int64_t)unit * DW_QMAX);
  k = k < 1 ? 1 : (k > 8 ? 8 : k);
  return unit * (int)k;
}
// (DW_TRUNK_JOBS = 7, struct DwTrunk: dw_pair.h)
__global__ void __launch_bounds__(512, 2)
mlp_bwd_dw6_trunk_kernel(int64_t P, DwTrunk J, const int* __restrict__ live_idx, const int* __restrict__ live_cnt, int ncu) {
  if (live_idx) P = (int64_t)__builtin_amdgcn_readfirstlane(*live_cnt);
  const int nact = dw_trunk_chunks(P, ncu);
  if ((int)blockIdx.x >= nact) return;
  const int job = (int)blockIdx.y;
  dw6_body<4, 2, 2, 4, true, false>(P, J.dY[job], J.X[job], nullptr, J.pw[job], J.pb[job], nullptr, live_idx, nullptr, nullptr,
                                    (int)blockIdx.x, nact);
}

// ---------------------------------------------------------------------------------------------------------------------
// The trunk jobs of BOTH passes of a two-net step in one launch (the paired backward: fn::x6_pair_* below, render.cpp rr_bwd).  A trunk workgroup
// holds 96 KiB of LDS, a CU runs one at a time, so a launch costs whole rounds of ncu workgroups: at 4096 rays x (64 + 192) samples the passes
// alone are 7 x 64 = 448 (1.75 rounds, costs 2) and 7 x 192 = 1344 workgroups (5.25 rounds, costs 6) of 256 k-steps each on 256 CUs; together they
// are 1792 = exactly 7 rounds.  ceil(7 (c0 + c1) / ncu) <= ceil(7 c0 / ncu) + ceil(7 c1 / ncu): no shape takes more rounds than the two launches.
// grid = 7 (c_fine + c_coarse) workgroups, flat, decoded to (pass, job, chunk) with the chunk fastest -- the dispatch order of the per-pass
// grid (chunks, 7), the fine pass first; c = dw_trunk_chunks(the pass's own point count).  No dead workgroups (a (max chunks, 14) grid with
// early exits would dispatch 896 of them at that shape).  Inside a job nothing differs from the per-pass launch: chunk count, k-step ranges and
// partial regions are the same, so the partials, and every gradient reduced from them, are bit-identical.  No live list: the compacted backward
// shares one act buffer between its passes and stays on the per-pass launch.
// ---------------------------------------------------------------------------------------------------------------------
struct DwTrunkPair {
  DwTrunk J[2];     // [0] the fine pass, [1] the coarse pass
  int64_t P[2];
};
__global__ void __launch_bounds__(512, 2)
mlp_bwd_dw6_trunk_pair_kernel(DwTrunkPair A, int ncu) {
  const int c0 = dw_trunk_chunks(A.P[0], ncu);
  int b = (int)blockIdx.x;
  const int pass = b >= DW_TRUNK_JOBS * c0 ? 1 : 0;
  if (pass) b -= DW_TRUNK_JOBS * c0;
  const int64_t P = A.P[pass];
  const int nact = pass ? dw_trunk_chunks(P, ncu) : c0;
  const int job = b / nact;
  if (job >= DW_TRUNK_JOBS) return;   // never taken while host and device agree on ncu (the grid is exactly 7 (c0 + c1)): it keeps a mismatch inside the job tables
  const DwTrunk& J = A.J[pass];
  dw6_body<4, 2, 2, 4, true, false>(P, J.dY[job], J.X[job], nullptr, J.pw[job], J.pb[job], nullptr, nullptr, nullptr, nullptr, b - job * nact,
                                    nact);
}

// rgb head + alpha bias gradients (VALU reduction over points): per-workgroup partials
//   out[wg][0..383] = dWr[c][k], [384..386] = dbr[c], [387] = dba
__global__ void __launch_bounds__(128) head_grads_kernel(int64_t P, const float* __restrict__ draw,
                                                          const float* __restrict__ hv,
                                                          float* __restrict__ partial, const int* __restrict__ live_idx,
                                                          const int* __restrict__ live_cnt) {
  const int k = threadIdx.x;
  if (live_idx) P = *live_cnt;
  auto dptr = [&](int64_t q) { return draw + (live_idx ? (int64_t)live_idx[q] : q) * 4; };
  const int64_t per = (P + gridDim.x - 1) / gridDim.x;
  const int64_t pa = blockIdx.x * per;
  int64_t pb = pa + per;
  if (pb > P) pb = P;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, sb = 0.f;
  int64_t p = pa;
  constexpr int NF = 16;   // independent points in flight (8 waves per CU: latency, not bandwidth, set the pace at 4); same sum order
  for (; p + NF <= pb; p += NF) {
    float4 d[NF];
    float h[NF];
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      d[i] = *reinterpret_cast<const float4*>(dptr(p + i));
      h[i] = hv[(p + i) * 128 + k];
    }
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      s0 = fmaf(d[i].x, h[i], s0); s1 = fmaf(d[i].y, h[i], s1); s2 = fmaf(d[i].z, h[i], s2);
      if (k < 4) sb += (k == 0) ? d[i].x : (k == 1) ? d[i].y : (k == 2) ? d[i].z : d[i].w;
    }
  }
  for (; p < pb; ++p) {
    const float4 d = *reinterpret_cast<const float4*>(dptr(p));
    const float h = hv[p * 128 + k];
    s0 = fmaf(d.x, h, s0); s1 = fmaf(d.y, h, s1); s2 = fmaf(d.z, h, s2);
    if (k < 4) sb += (k == 0) ? d.x : (k == 1) ? d.y : (k == 2) ? d.z : d.w;
  }
  float* o = partial + (int64_t)blockIdx.x * 388;
  o[k] = s0; o[128 + k] = s1; o[256 + k] = s2;
  if (k < 4) o[384 + k] = sb;
}

// ---------------------------------------------------------------------------------------------------------------------
// The same 388 values from the dX kernel (fp32 / bf16x6): phase A of mlp_bwd_dx_kernel holds hv and draw of its tile anyway and leaves one
// row of 388 sums per 64-point TILE in a workspace the library owns (fn::head_workspace below), so head_grads_kernel's second pass over hv
// and draw (0.55 GB per step at the bench shape) is not made.  head_group_kernel sums groups of G consecutive tiles, in ascending tile order,
// into at most HEAD_ROWS rows of the head region, which reduce_all then walks like any other job's chunks.  G and the row count are functions
// of the POINT COUNT ALONE (the tile scheduler of dX is dynamic: which workgroup ran a tile must not matter, and does not), so the live-list
// backward -- tiles of the list, count on the device -- equals the plain backward of the same points bit for bit.
// HEAD_ROWS = 256: reduce_all sums a column through nwg / 16 dependent rounds of loads, 16 for this segment as for a trunk job.
// ---------------------------------------------------------------------------------------------------------------------
#define HEAD_ROWS 256
__host__ __device__ static inline int head_group(int64_t ntiles) {   // tiles per row
  const int64_t g = (ntiles + HEAD_ROWS - 1) / HEAD_ROWS;
  return g < 1 ? 1 : (int)g;
}
__host__ __device__ static inline int head_rows(int64_t P) {
  const int64_t ntiles = (P + TM - 1) / TM;
  const int g = head_group(ntiles);
  return (int)((ntiles + g - 1) / g);
}
// grid (min(tiles of the capacity, HEAD_ROWS), 4) x 128: one output per thread, NF independent loads in flight, added in ascending tile order
__global__ void __launch_bounds__(128) head_group_kernel(int64_t P, const float* __restrict__ ws, float* __restrict__ out,
                                                          const int* __restrict__ live_cnt) {
  if (live_cnt) P = (int64_t)*live_cnt;
  const int64_t ntiles = (P + TM - 1) / TM;
  const int g = head_group(ntiles);
  const int col = (int)blockIdx.y * 128 + (int)threadIdx.x;
  const int64_t t0 = (int64_t)blockIdx.x * g;
  if (t0 >= ntiles || col >= 388) return;
  const int n = (int)(ntiles - t0 < g ? ntiles - t0 : g);
  const float* src = ws + t0 * 388 + col;
  constexpr int NF = 16;
  float s = 0.f;
  int i = 0;
  for (; i + NF <= n; i += NF) {
    float v[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) v[j] = src[(int64_t)(i + j) * 388];
#pragma unroll
    for (int j = 0; j < NF; ++j) s += v[j];
  }
  for (; i < n; ++i) s += src[(int64_t)i * 388];
  out[(int64_t)blockIdx.x * 388 + col] = s;
}

// ---- one launch reduces every job's per-workgroup partials into the flat gradient ------------
// (struct RedSeg, MAX_SEGS, struct RedTable: dw_pair.h)

__global__ void __launch_bounds__(256) reduce_all_kernel(RedTable tab, const float* __restrict__ partial, float* __restrict__ grads,
                                                          float* __restrict__ scratch, int64_t P, const int* __restrict__ live_cnt, int ncu) {
  RedSeg sg = tab.s[blockIdx.y];
  if (sg.dyn) {
    if (live_cnt) P = (int64_t)*live_cnt;
    const int n = sg.dyn == 2 ? head_rows(P) : dw_trunk_chunks(P, ncu);
    sg.nwg = n < sg.nwg ? n : sg.nwg;
  }
  const int64_t total = (int64_t)sg.rows * sg.cols;
  const float* src = partial + sg.src;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(e / sg.cols), c = (int)(e % sg.cols);
    if (c >= sg.valid_cols) continue;
    // RS running sums (chunk w goes to sum w mod RS), combined pairwise: a fixed order that depends on the chunk count alone, and RS independent
    // loads in flight per lane -- the kernel is a chain of dependent HBM round trips, not a bandwidth problem (round 6; it was 5 % of the 512-ray step)
    constexpr int RS = 16;      // (32 measured 6x SLOWER: 46 -> 277 us at 512 rays -- the loads of a round no longer issue back to back)
    float a[RS];
#pragma unroll
    for (int i = 0; i < RS; ++i) a[i] = 0.f;
    int w = 0;
    for (; w + RS <= sg.nwg; w += RS) {
#pragma unroll
      for (int i = 0; i < RS; ++i) a[i] += src[(int64_t)(w + i) * sg.wg_stride + e];
    }
#pragma unroll
    for (int i = 0; i < RS - 1; ++i)      // (the tail: chunk counts are multiples of ncu / 8, the head-gradient grid of 1024 -- normally empty)
      if (w + i < sg.nwg) a[i] += src[(int64_t)(w + i) * sg.wg_stride + e];
#pragma unroll
    for (int h = RS / 2; h >= 1; h >>= 1)
#pragma unroll
      for (int i = 0; i < h; ++i) a[i] += a[i + h];
    if (c < sg.sc_cols) scratch[sg.sc_dst + (int64_t)r * sg.sc_cols + c] = a[0];
    else grads[sg.dst + (int64_t)r * sg.ld + c] = a[0];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The unfold: the gradients of the two layers that the kernels run as one (M = Wv_a Wf, Wv_a = Wv[:, :256]; mlp_pack.hip fold_kernel) from
// G = dL/dM [128][256] (the view job's h7 columns, reduced into scratch), dbv (already in the flat gradient) and the current weights:
//   dWf = Wv_a^T G  [256][256],   dbf = Wv_a^T dbv  [256],   dWv_a = G Wf^T + dbv bf^T  [128][256]
// fp64 products and sums in ascending k, one rounding to fp32: parameter-sized work (2 x 8.4 M FMAs), one launch per pass behind reduce_all.
// 16 x 16 output tiles, operands staged through LDS 16 k at a time; blocks 0..255 dWf, 256..383 dWv_a, 384 dbf.
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) unfold_kernel(const float* __restrict__ G, const float* __restrict__ params, float* __restrict__ grads,
                                                      int64_t VW, int64_t VB, int64_t FW, int64_t FB) {
  __shared__ double As[16][17], Bs[16][17];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int b = blockIdx.x;
  if (b == 384) {   // dbf[i] = sum_o Wv[o][i] dbv[o]
    const int i = threadIdx.x;
    double s = 0.0;
    for (int o = 0; o < 128; ++o) s = fma((double)params[VW + (int64_t)o * 283 + i], (double)grads[VB + o], s);
    grads[FB + i] = (float)s;
    return;
  }
  const bool wf = b < 256;                       // dWf tile (i0, j0) / dWv_a tile (o0, i0)
  const int r0 = wf ? (b >> 4) * 16 : ((b - 256) >> 4) * 16, c0 = (b & 15) * 16;
  const int K = wf ? 128 : 256;
  double s = 0.0;
  for (int k0 = 0; k0 < K; k0 += 16) {
    if (wf) {   // A[k][r] = Wv[k][r0 + r], B[k][c] = G[k][c0 + c]
      As[ty][tx] = (double)params[VW + (int64_t)(k0 + ty) * 283 + r0 + tx];
      Bs[ty][tx] = (double)G[(k0 + ty) * 256 + c0 + tx];
    } else {    // A[k][r] = G[r0 + r][k], B[k][c] = Wf[c0 + c][k]
      As[tx][ty] = (double)G[(r0 + ty) * 256 + k0 + tx];
      Bs[tx][ty] = (double)params[FW + (int64_t)(c0 + ty) * 256 + k0 + tx];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) s = fma(As[k][ty], Bs[k][tx], s);
    __syncthreads();
  }
  if (wf) grads[FW + (int64_t)(r0 + ty) * 256 + c0 + tx] = (float)s;
  else grads[VW + (int64_t)(r0 + ty) * 283 + c0 + tx] = (float)fma((double)grads[VB + r0 + ty], (double)params[FB + c0 + tx], s);
}

// (the dW jobs of one net and their partial regions -- DwJobDesc, dw_job, dw_job_base: dw_pair.h)
extern "C" int64_t fastnerf_mlp_bwd_partial_floats(void) {
  return dw_partial_floats(fn::device_cus());
}

template <int WO, int WI, int TO, int TI, bool BIAS, bool RANK1, int MM = MM_F32, int CTI2 = 0, int CTO2 = 0>
static int launch_dw(int64_t P, const float* dY, int ldy, const float* X, int ldx, const float* draw, float* base,
                     int nwg, hipStream_t st, const int* live_idx = nullptr, const int* live_cnt = nullptr,
                     const float* X2 = nullptr, const float* dY2 = nullptr, float* pr_at = nullptr) {
  constexpr int NO = WO * TO * 32, KI = WI * TI * 32;
  float* pw = base;
  float* pb = base + (int64_t)nwg * NO * KI;
  float* pr = pr_at ? pr_at : pb + (BIAS ? (int64_t)nwg * (NO - CTO2 * 32) : 0);   // pr_at: the rank-1 partials live elsewhere
  if constexpr (MM == MM_X6) {
    if (ldy != NO - CTO2 * 32 || ldx != KI - CTI2 * 32 || (CTI2 > 0) != (X2 != nullptr) || (CTO2 > 0) != (dY2 != nullptr)) {
      fn::set_error("launch_dw: the bf16x6 dW kernel needs ld == width (and X2 / dY2 exactly when CTI2 / CTO2 > 0)");
      return -1;
    }
    constexpr int lds6 = 2 * (WO * TO + WI * TI) * 3 * 1024 + 128;
    auto kern6 = mlp_bwd_dw6_kernel<WO, WI, TO, TI, BIAS, RANK1, CTI2, CTO2>;
    static fn::DevOnce once6;
    if (int rc = fn::set_dyn_lds(reinterpret_cast<const void*>(kern6), once6, lds6)) return rc;
    hipLaunchKernelGGL(kern6, dim3(nwg), dim3(WO * WI * 64), lds6, st, P, dY, X, draw, pw, pb, pr, live_idx, live_cnt, X2, dY2);
    FN_LAUNCH_CHECK();
    return 0;
  } else {
    static_assert(MM == MM_F32 && CTI2 == 0 && CTO2 == 0, "two-tensor jobs exist for the bf16x6 dW kernel only");
    constexpr int STAGE = DW_MT * (NO + KI) + DW_MT;
    const size_t lds = 2 * STAGE * sizeof(float);
    auto kern = mlp_bwd_dw_kernel<WO, WI, TO, TI, BIAS, RANK1>;
    static fn::DevOnce once;
    if (int rc = fn::set_dyn_lds(reinterpret_cast<const void*>(kern), once, (int)lds)) return rc;
    hipLaunchKernelGGL(kern, dim3(nwg), dim3(WO * WI * 64), lds, st, P, dY, ldy, X, ldx, draw, pw, pb, pr, live_idx, live_cnt);
    FN_LAUNCH_CHECK();
    return 0;
  }
}

// the rebuilding view job: launch_dw's partial layout and grid
template <int WO, int WI, int TO, int TI, bool BIAS, bool RANK1, int CTI2>
static int launch_dw_rbv(int64_t P, const float* hv, const float* X, const float* draw, float* base, int nwg, hipStream_t st, const float* X2,
                         float* pr_at, const float* wr) {
  constexpr int NO = WO * TO * 32, KI = WI * TI * 32;
  float* pw = base;
  float* pb = base + (int64_t)nwg * NO * KI;
  float* pr = pr_at ? pr_at : pb + (BIAS ? (int64_t)nwg * NO : 0);
  constexpr int lds6 = 2 * (WO * TO + WI * TI) * 3 * 1024 + 128 + 512;   // + DR: [2][16] float4
  auto kern = mlp_bwd_dw6_rbv_kernel<WO, WI, TO, TI, BIAS, RANK1, CTI2>;
  static fn::DevOnce once;
  if (int rc = fn::set_dyn_lds(reinterpret_cast<const void*>(kern), once, lds6)) return rc;
  hipLaunchKernelGGL(kern, dim3(nwg), dim3(WO * WI * 64), lds6, st, P, hv, X, draw, pw, pb, pr, X2, wr);
  FN_LAUNCH_CHECK();
  return 0;
}

static void add_seg(RedTable& T, int64_t src, int64_t wg_stride, int nwg, int rows, int cols, int64_t dst, int ld,
                    int valid_cols, int dyn = 0, int sc_cols = 0, int64_t sc_dst = 0) {
  RedSeg& s = T.s[T.n++];
  s.src = src; s.wg_stride = wg_stride; s.nwg = nwg; s.rows = rows; s.cols = cols; s.dst = dst; s.ld = ld;
  s.valid_cols = valid_cols; s.dyn = dyn; s.sc_cols = sc_cols; s.sc_dst = sc_dst;
}

// the trunk entries need 96 KiB of dynamic LDS (fn::set_dyn_lds)
constexpr int DW_TRUNK_LDS = 2 * 16 * 3 * 1024 + 128;
// a job's partial region holds nwg chunks: on a part with fewer than 8 CUs dw_trunk_chunks can ask for more
static int trunk_chunks_fit(int64_t P, int ncu, int nwg) {
  if (dw_trunk_chunks(P, ncu) > nwg) {
    fn::set_error("mlp_bwd: the trunk launch needs %d chunks per job, the partial regions hold %d (a device with fewer than 8 CUs?)",
                  dw_trunk_chunks(P, ncu), nwg);
    return -1;
  }
  return 0;
}

// (struct DwDeferred -- what a pass of the paired backward leaves undone: dw_pair.h)
// reduce_all + unfold of one pass: the partials of every job into the flat gradient, then G = dL/dM into the two folded layers' gradients
static int bwd_reduce(const RedTable& T, const NetLayout& L, int64_t P, const float* params, float* partial, float* grads, int64_t g_off,
                      const int* live_cnt, int ncu, hipStream_t st) {
  hipLaunchKernelGGL(reduce_all_kernel, dim3(256, T.n), dim3(256), 0, st, T, partial, grads, partial, P, live_cnt, ncu);   // (256 x 256 threads: one element of a 256 x 256 segment per lane)
  FN_LAUNCH_CHECK();
  hipLaunchKernelGGL(unfold_kernel, dim3(385), dim3(256), 0, st, partial + g_off, params, grads, L.VW, L.VB, L.FW, L.FB);
  FN_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// The per-tile head partials [tiles][388] of the dX kernel: a workspace the library owns (fn::stream_ws, slot WS_HEAD_TILES).  388 floats per
// 64 points: 19.1 MB for the fine pass of the bench shape (12 288 tiles), which the coarse pass (4 096 tiles) of the same stream reuses behind
// it.  nullptr -- no workspace (a capturing stream, no memory), or FASTNERF_HEAD_FROM_DX=0 in the environment (read at every call: the switch
// the tests compare the two routes with) -- sends the caller down the head_grads_kernel route.  (FASTNERF_HEAD_FROM_DX=nan, also for the tests:
// the buffer is filled with NaNs before dX writes it: every value read was written.)
// ---------------------------------------------------------------------------------------------------------------------
namespace fn {
static float* head_workspace(int64_t ntiles, hipStream_t st) {
  const char* e = getenv("FASTNERF_HEAD_FROM_DX");
  if (e && e[0] == '0') return nullptr;
  static const WsName what = {
      "fastnerf: no memory for the per-tile head partials of the backward (%.1f MB): this stream keeps the head_grads launch\n", 1e-6};
  const StreamWs w = stream_ws(WS_HEAD_TILES, st, (ntiles > 0 ? ntiles : 1) * 388, what);
  if (w.p && e && e[0] == 'n') (void)hipMemsetAsync(w.p, 0xFF, sizeof(float) * (size_t)w.cap, st);
  return w.p;
}
}  // namespace fn

// ---------------------------------------------------------------------------------------------------------------------
// FASTNERF_SIDE_REBUILD, read at every call like FASTNERF_HEAD_FROM_DX: unset / anything else -- a caller that can (render.cpp, the fused step in
// bf16x6 on the plain backward) lets the view job rebuild dYv and stops dX's store of it;  0 -- the reading route, the store on;  nan -- the
// rebuilding route with dact_yv filled with NaNs first: nobody reads it.
// ---------------------------------------------------------------------------------------------------------------------
static std::atomic<int64_t> g_rebuild_passes{0};
namespace fn {
int side_rebuild_mode(void) {   // 0: off, 1: on, 2: on + poison
  const char* e = getenv("FASTNERF_SIDE_REBUILD");
  if (e && e[0] == '0') return 0;
  return (e && e[0] == 'n') ? 2 : 1;
}
}  // namespace fn

template <int MM>
static int bwd_launch_t(int kind, int64_t n, int S, const float* draw, const float* act, const float* params,
                      const float* packed_bwd, float* dact, float* partial, float* grads, const int* live_idx,
                      const int* live_cnt, fn_stream_t stream, DwDeferred* defer = nullptr, const SideRb* rb = nullptr) {
  constexpr int MW = MM;
  const NetLayout& L = layout_of(kind);
  const int PEP = L.pe_pad;
  hipStream_t st = fn::S(stream);
  const int64_t P = n * S;
  const int64_t ntiles = (P + TM - 1) / TM;
  const int ncu = fn::device_cus();
  int grid = ncu * WG_PER_CU;
  if (ntiles < grid) grid = (int)ntiles;
  float* const headws = fn::head_workspace(ntiles, st);   // nullptr: the rgb-head / alpha-bias gradients take their own pass below
  // the rebuilding view job (dw6_body RBV): bf16x6, the 64-channel encoding, no list
  if (rb && (MM != MM_X6 || PEP != 64 || live_idx)) {
    fn::set_error("mlp_bwd: the rebuilding view job needs bf16x6, the 64-channel encoding and no live list");
    return -1;
  }
  if (rb) g_rebuild_passes.fetch_add(1, std::memory_order_relaxed);
  if (rb && rb->poison) (void)hipMemsetAsync(dact + dact_yv(P), 0xFF, sizeof(float) * (size_t)P * 128, st);
  if (int rc_dx = fn_launch_dx(MM, grid, st, P, draw, act, params, packed_bwd, dact, L, live_idx, live_cnt, headws,
                               (rb && rb->no_store) ? FN_DX_NO_DYV_STORE : 0))
    return rc_dx;

  // ---- dW jobs: every job writes per-chunk partials into its own region ------------------
  // (grids and chunk counts are functions of the point count alone -- one workgroup per CU and a fixed head-gradient grid for the jobs with
  // their own launch, dw_trunk_chunks for the seven 256 x 256 jobs of the bf16x6 trunk launch -- so the order in which partial sums meet
  // depends on the point count only: live-list backward == plain backward of the same points, bit for bit)
  const int nwg = ncu;
  RedTable T;
  T.n = 0;
  int rc;
  const float* a_pe = act + act_pe(P, PEP);
  auto region = [&](int j) { return partial + dw_job_base(j, ncu, PEP); };
  auto segs = [&](int j, int64_t dstW, int ld, int validc, int64_t dstB, int64_t dstR, int dyn = 0) {
    const DwJobDesc d = dw_job(j, PEP);
    const int64_t b = dw_job_base(j, ncu, PEP);
    add_seg(T, b, (int64_t)d.NO * d.KI, nwg, d.NO, d.KI, dstW, ld, validc, dyn);
    int64_t o = b + (int64_t)nwg * d.NO * d.KI;
    if (d.bias) { add_seg(T, o, d.NO, nwg, 1, d.NO, dstB, d.NO, d.NO, dyn); o += (int64_t)nwg * d.NO; }
    if (d.rank1) add_seg(T, o, d.KI, nwg, 1, d.KI, dstR, d.KI, d.KI, dyn);
  };
  // L0 (+ L5's pe part in the same job under MM_X6: one read and one split of the positional encoding for both;
  //     8 waves x (64 outputs x all pe tiles), partials [512][pe] + bias [256] across the neighbouring regions of jobs 0 and 8)
  if constexpr (MW == MM_X6) {
    // (16 waves x one X tile each for the 64-channel encoding: 225 us against 243 for 8 waves x both tiles, 326 for 4 waves -- the job is HBM-latency-bound, more waves in flight win; `tools/ab_kstats.sh`, round 6)
    if (PEP == 64) rc = launch_dw<8, 2, 2, 1, true, false, MW, 0, 8>(P, dact + dact_y(P, 0), 256, a_pe, 64, nullptr, region(0), nwg, st, live_idx, live_cnt, nullptr, dact + dact_y(P, 5));
    else rc = launch_dw<8, 1, 2, 3, true, false, MW, 0, 8>(P, dact + dact_y(P, 0), 256, a_pe, 96, nullptr, region(0), nwg, st, live_idx, live_cnt, nullptr, dact + dact_y(P, 5));
    if (rc) return rc;
    const int64_t b0 = dw_job_base(0, ncu, PEP);
    add_seg(T, b0, (int64_t)512 * PEP, nwg, 256, PEP, L.LW[0], L.in_pe, L.in_pe);
    add_seg(T, b0 + (int64_t)256 * PEP, (int64_t)512 * PEP, nwg, 256, PEP, L.LW[5], 256 + L.in_pe, L.in_pe);
    add_seg(T, b0 + (int64_t)nwg * 512 * PEP, 256, nwg, 1, 256, L.LB[0], 256, 256);
  } else {
    if (PEP == 64) rc = launch_dw<4, 1, 2, 2, true, false, MW>(P, dact + dact_y(P, 0), 256, a_pe, 64, nullptr, region(0), nwg, st, live_idx, live_cnt);
    else rc = launch_dw<4, 1, 2, 3, true, false, MW>(P, dact + dact_y(P, 0), 256, a_pe, 96, nullptr, region(0), nwg, st, live_idx, live_cnt);
    if (rc) return rc;
    segs(0, L.LW[0], L.in_pe, L.in_pe, L.LB[0], 0);
  }
  // L1..L7 (h part); MM_X6: the trunk launch below
  if constexpr (MW != MM_X6) {
    for (int l = 1; l < 8; ++l) {
      if ((rc = launch_dw<4, 2, 2, 4, true, false, MW>(P, dact + dact_y(P, l), 256, act + act_h(P, PEP, l - 1), 256, nullptr, region(l), nwg, st, live_idx, live_cnt))) return rc;
      segs(l, L.LW[l] + (l == 5 ? L.in_pe : 0), l == 5 ? 256 + L.in_pe : 256, 256, L.LB[l], 0);
    }
  }
  // L5 pe part (MM_X6: done with L0 above)
  if constexpr (MW != MM_X6) {
    if (PEP == 64) rc = launch_dw<4, 1, 2, 2, false, false, MW>(P, dact + dact_y(P, 5), 256, a_pe, 64, nullptr, region(8), nwg, st, live_idx, live_cnt);
    else rc = launch_dw<4, 1, 2, 3, false, false, MW>(P, dact + dact_y(P, 5), 256, a_pe, 96, nullptr, region(8), nwg, st, live_idx, live_cnt);
    if (rc) return rc;
    segs(8, L.LW[5], 256 + L.in_pe, L.in_pe, 0, 0);
  }
  // L1..L7 under MM_X6: the trunk launch; chunk w of a job writes where workgroup w of its own launch did
  if constexpr (MW == MM_X6) {
    DwTrunk J;
    for (int l = 1; l < 8; ++l) {
      J.dY[l - 1] = dact + dact_y(P, l);
      J.X[l - 1] = act + act_h(P, PEP, l - 1);
      J.pw[l - 1] = region(l);
      J.pb[l - 1] = region(l) + (int64_t)nwg * 256 * 256;
    }
    if ((rc = trunk_chunks_fit(P, ncu, nwg))) return rc;
    if (defer) {
      defer->J = J;   // (the paired backward: one launch for both passes, fn::x6_pair_finish)
    } else {
      static fn::DevOnce once_t;
      if ((rc = fn::set_dyn_lds(reinterpret_cast<const void*>(mlp_bwd_dw6_trunk_kernel), once_t, DW_TRUNK_LDS))) return rc;
      hipLaunchKernelGGL(mlp_bwd_dw6_trunk_kernel, dim3(dw_trunk_chunks(P, ncu), DW_TRUNK_JOBS), dim3(512), DW_TRUNK_LDS, st, P, J, live_idx, live_cnt, ncu);
      FN_LAUNCH_CHECK();
    }
    for (int l = 1; l < 8; ++l) segs(l, L.LW[l] + (l == 5 ? L.in_pe : 0), l == 5 ? 256 + L.in_pe : 256, 256, L.LB[l], 0, 1);
  }
  // view layer on [h7 | vpe] (the folded feature / remap layer: mlp_pack.hip), with the alpha / sigma head as a rank-1 row over h7.
  // The h7 columns of its dW are G = dL/dM: reduce_all leaves them in scratch (the former feature job's region, behind the rank-1
  // partials), and unfold_kernel turns G into dWf, dbf and dWv[:, :256] below.
  float* const pr_view = region(9);
  const int64_t g_off = dw_job_base(9, ncu, PEP) + (int64_t)nwg * 256;
  if constexpr (MW == MM_X6) {
    // one job for both inputs of the view layer (h7 [P,256] | encoded direction [P,32]): dYv is read and split once; 12 waves,
    // partials [128][288] + bias [128] across the (adjacent) regions of jobs 10 and 11
    if (rb) rc = launch_dw_rbv<4, 3, 1, 3, true, true, 1>(P, act + act_hv(P, PEP), act + act_h(P, PEP, 7), draw, region(10), nwg, st, act + act_vpe(P, PEP),
                                                          pr_view, params + L.RW);
    else rc = launch_dw<4, 3, 1, 3, true, true, MW, 1, 0>(P, dact + dact_yv(P), 128, act + act_h(P, PEP, 7), 256, draw, region(10), nwg, st,
                                                    live_idx, live_cnt, act + act_vpe(P, PEP), nullptr, pr_view);
    if (rc) return rc;
    const int64_t b10 = dw_job_base(10, ncu, PEP);
    add_seg(T, b10, 128 * 288, nwg, 128, 288, L.VW, 283, 283, 0, 256, g_off);
    add_seg(T, b10 + (int64_t)nwg * 128 * 288, 128, nwg, 1, 128, L.VB, 128, 128);
  } else {
    if ((rc = launch_dw<2, 4, 2, 2, true, true, MW>(P, dact + dact_yv(P), 128, act + act_h(P, PEP, 7), 256, draw, region(10), nwg, st, live_idx, live_cnt,
                                              nullptr, nullptr, pr_view))) return rc;
    const int64_t b10 = dw_job_base(10, ncu, PEP);
    add_seg(T, b10, 128 * 256, nwg, 128, 256, L.VW, 283, 256, 0, 256, g_off);
    add_seg(T, b10 + (int64_t)nwg * 128 * 256, 128, nwg, 1, 128, L.VB, 128, 128);
    if ((rc = launch_dw<4, 1, 1, 1, false, false, MW>(P, dact + dact_yv(P), 128, act + act_vpe(P, PEP), 32, nullptr, region(11), nwg, st, live_idx, live_cnt))) return rc;
    segs(11, L.VW + 256, 283, 27, 0, 0);
  }
  add_seg(T, dw_job_base(9, ncu, PEP), 256, nwg, 1, 256, L.AW, 256, 256);   // dWa: the rank-1 row
  // rgb head + alpha bias: the per-tile sums that dX left in headws, grouped into rows of the head region; without a workspace, their own pass
  if (headws != nullptr) {
    const int64_t hb = dw_job_base(12, ncu, PEP);
    const int rows = ntiles < HEAD_ROWS ? (int)ntiles : HEAD_ROWS;   // (live list: the rows of the capacity; head_rows(live count) of them are written and reduced)
    hipLaunchKernelGGL(head_group_kernel, dim3(rows, 4), dim3(128), 0, st, P, headws, partial + hb, live_cnt);
    FN_LAUNCH_CHECK();
    add_seg(T, hb, 388, rows, 1, 388, L.RW, 388, 387, 2);   // dWr (384) + dbr (3), contiguous in every layout
    add_seg(T, hb + 387, 388, rows, 1, 1, L.AB, 1, 1, 2);   // dba
  } else {
    const int hg = HEAD_MAX_WG;
    const int64_t hb = dw_job_base(12, ncu, PEP);
    hipLaunchKernelGGL(head_grads_kernel, dim3(hg), dim3(128), 0, st, P, draw, act + act_hv(P, PEP), partial + hb, live_idx, live_cnt);
    FN_LAUNCH_CHECK();
    add_seg(T, hb, 388, hg, 1, 388, L.RW, 388, 387);   // dWr (384) + dbr (3), contiguous in every layout
    add_seg(T, hb + 387, 388, hg, 1, 1, L.AB, 1, 1);   // dba
  }
  if (defer) {
    defer->T = T; defer->P = P; defer->g_off = g_off; defer->params = params; defer->partial = partial; defer->grads = grads; defer->kind = kind;
    return 0;
  }
  return bwd_reduce(T, L, P, params, partial, grads, g_off, live_cnt, ncu, st);
}

// ---------------------------------------------------------------------------------------------------------------------
// The paired bf16x6 backward (render.cpp rr_bwd: one call runs both passes of a two-net step on the saving route).  Order on the stream:
//   fine pass:   dX (+ per-tile head sums), pe job, view job, head_group      (x6_pair_pass: the caller's dact / partial workspaces)
//   coarse pass: the same                                   (x6_pair_pass: the SIDE dact / partial set below)
//   ONE trunk launch over the 14 jobs of both passes        (x6_pair_finish)
//   reduce_all + unfold of the fine net, then of the coarse net
// The fine pass's dact and partials must survive the coarse pass, so the coarse pass gets a second dact + partial set that the library owns
// (fn::stream_ws, slots WS_PAIR_DACT and WS_PAIR_PARTIAL): dact of the coarse pass's points (9.7 KB per point) + one partial buffer, 2.55 GB +
// 0.63 GB at 4096 x 64 coarse points on a 256-CU part.  Without it (a capturing stream, no memory) x6_pair_workspace returns false, which is
// no error: the caller takes the unpaired route -- the same kernels on the same data, bit-identical gradients.
// ---------------------------------------------------------------------------------------------------------------------
namespace fn {
static std::atomic<int64_t> g_pair_launches{0};

// the side dact / partial set of this (device, stream) for a coarse pass of P_coarse points; false: take the unpaired route
bool x6_pair_workspace(int64_t P_coarse, fn_stream_t stream, float** dact2, float** partial2) {
  static const WsName what = {
      "fastnerf: no memory for the side workspace of the paired bf16x6 backward (%.2f GB): this stream keeps the per-pass trunk launches\n", 1e-9};
  const StreamWs d = stream_ws(WS_PAIR_DACT, S(stream), P_coarse * (int64_t)DACT_FLOATS, what);
  if (!d.p) return false;
  const StreamWs p = stream_ws(WS_PAIR_PARTIAL, S(stream), fastnerf_mlp_bwd_partial_floats(), what);
  if (!p.p) return false;
  *dact2 = d.p;
  *partial2 = p.p;
  return true;
}

// everything of fastnerf_mlp_x6_bwd but the trunk launch, the reduction and the unfold, which it records in *d (the caller's, one per pass)
// rb: NULL, or the rebuilding view job (dw_pair.h SideRb)
int x6_pair_pass(DwDeferred* d, int64_t n, int S, const float* draw, const float* act, const float* params, const float* packed_bwd,
                 float* dact, float* partial, float* grads, fn_stream_t stream, const SideRb* rb) {
  FN_CHECK_ARG(d && n > 0 && S >= 1, "d != NULL, n>0, S>=1");
  FN_CHECK_ARG(draw && act && params && packed_bwd && dact && partial && grads, "null pointer");
  return bwd_launch_t<MM_X6>(0, n, S, draw, act, params, packed_bwd, dact, partial, grads, nullptr, nullptr, stream, d, rb);
}
// fastnerf_mlp_x6_bwd(kind 0) with the rebuilding view job: a whole pass, trunk launch, reduction and unfold included
int x6_bwd_rebuild(int64_t n, int S, const float* draw, const float* act, const float* params, const float* packed_bwd, float* dact,
                   float* partial, float* grads, fn_stream_t stream, const SideRb* rb) {
  FN_CHECK_ARG(n > 0 && S >= 1 && rb, "n>0, S>=1, rb != NULL");
  FN_CHECK_ARG(draw && act && params && packed_bwd && dact && partial && grads, "null pointer");
  return bwd_launch_t<MM_X6>(0, n, S, draw, act, params, packed_bwd, dact, partial, grads, nullptr, nullptr, stream, nullptr, rb);
}

// ONE trunk launch over both passes, then each net's reduction and unfold
int x6_pair_finish(const DwDeferred* fine, const DwDeferred* coarse, fn_stream_t stream) {
  hipStream_t st = S(stream);
  const int ncu = fn::device_cus();
  const DwDeferred* d[2] = {fine, coarse};
  DwTrunkPair A;
  int nwg = 0;
  for (int k = 0; k < 2; ++k) {
    A.J[k] = d[k]->J;
    A.P[k] = d[k]->P;
    nwg += DW_TRUNK_JOBS * dw_trunk_chunks(A.P[k], ncu);   // (each count fits its regions: bwd_launch_t has checked)
  }
  static DevOnce once_p;
  if (int rc = set_dyn_lds(reinterpret_cast<const void*>(mlp_bwd_dw6_trunk_pair_kernel), once_p, DW_TRUNK_LDS)) return rc;
  hipLaunchKernelGGL(mlp_bwd_dw6_trunk_pair_kernel, dim3(nwg), dim3(512), DW_TRUNK_LDS, st, A, ncu);
  FN_LAUNCH_CHECK();
  g_pair_launches.fetch_add(1, std::memory_order_relaxed);
  for (int k = 0; k < 2; ++k)
    if (int rc = bwd_reduce(d[k]->T, layout_of(d[k]->kind), d[k]->P, d[k]->params, d[k]->partial, d[k]->grads, d[k]->g_off, nullptr, ncu, st)) return rc;
  return 0;
}
}  // namespace fn
// paired trunk launches this process has enqueued: tells a caller (and tests/test_gpu_trunk_pair.py) which route its backward took
extern "C" int64_t fastnerf_x6_pair_launches(void) { return fn::g_pair_launches.load(std::memory_order_relaxed); }
// backward passes with a rebuilding view job this process has enqueued (tests/test_gpu_side_rebuild.py)
extern "C" int64_t fastnerf_side_rebuild_passes(void) { return g_rebuild_passes.load(std::memory_order_relaxed); }

static int bwd_launch(int kind, int64_t n, int S, const float* draw, const float* act, const float* params,
                      const float* packed_bwd, float* dact, float* partial, float* grads, const int* live_idx,
                      const int* live_cnt, fn_stream_t stream, int mm = MM_F32) {
  return mm == MM_X6 ? bwd_launch_t<MM_X6>(kind, n, S, draw, act, params, packed_bwd, dact, partial, grads, live_idx, live_cnt, stream)
                     : bwd_launch_t<MM_F32>(kind, n, S, draw, act, params, packed_bwd, dact, partial, grads, live_idx, live_cnt, stream);
}
extern "C" int fastnerf_mlp_bwd_ex(int kind, int64_t n, int S, const float* draw, const float* act,
                                   const float* params, const float* packed_bwd, float* dact, float* partial,
                                   float* grads, fn_stream_t stream) {
  FN_CHECK_ARG(kind >= 0 && kind <= 2 && n > 0 && S >= 1, "kind in 0..2, n>0, S>=1");
  FN_CHECK_ARG(draw && act && params && packed_bwd && dact && partial && grads, "null pointer");
  return bwd_launch(kind, n, S, draw, act, params, packed_bwd, dact, partial, grads, nullptr, nullptr, stream);
}
// exact-fp32 twin of fastnerf_mlp_bf16_bwd_live
extern "C" int fastnerf_mlp_bwd_live_ex(int kind, int64_t n, int S, const float* draw, const float* act,
                                        const float* params, const float* packed_bwd, float* dact, float* partial,
                                        float* grads, const int32_t* live_idx, const int32_t* live_cnt,
                                        fn_stream_t stream) {
  FN_CHECK_ARG(kind >= 0 && kind <= 2 && n > 0 && S >= 1, "kind in 0..2, n>0, S>=1");
  FN_CHECK_ARG(draw && act && params && packed_bwd && dact && partial && grads && live_idx && live_cnt, "null pointer");
  return bwd_launch(kind, n, S, draw, act, params, packed_bwd, dact, partial, grads, live_idx, live_cnt, stream);
}
extern "C" int fastnerf_mlp_bwd(int64_t n, int S, const float* draw, const float* act, const float* params,
                                const float* packed_bwd, float* dact, float* partial, float* grads,
                                fn_stream_t stream) {
  return fastnerf_mlp_bwd_ex(0, n, S, draw, act, params, packed_bwd, dact, partial, grads, stream);
}

// ---- MM_X6 ("bf16x6") entry points: the call protocol of fastnerf_mlp_{fwd,bwd}_ex / _live_ex / _flags_ex, weights from
// fastnerf_mlp_x6_pack; saved activations and gradient workspaces have the exact-fp32 kernels' layouts and sizes.
extern "C" int fastnerf_mlp_x6_bwd(int kind, int64_t n, int S, const float* draw, const float* act, const float* params,
                                   const float* packed_bwd, float* dact, float* partial, float* grads, fn_stream_t stream) {
  FN_CHECK_ARG(kind >= 0 && kind <= 2 && n > 0 && S >= 1, "kind in 0..2, n>0, S>=1");
  FN_CHECK_ARG(draw && act && params && packed_bwd && dact && partial && grads, "null pointer");
  return bwd_launch(kind, n, S, draw, act, params, packed_bwd, dact, partial, grads, nullptr, nullptr, stream, MM_X6);
}
extern "C" int fastnerf_mlp_x6_bwd_live(int kind, int64_t n, int S, const float* draw, const float* act, const float* params,
                                        const float* packed_bwd, float* dact, float* partial, float* grads,
                                        const int32_t* live_idx, const int32_t* live_cnt, fn_stream_t stream) {
  FN_CHECK_ARG(kind >= 0 && kind <= 2 && n > 0 && S >= 1, "kind in 0..2, n>0, S>=1");
  FN_CHECK_ARG(draw && act && params && packed_bwd && dact && partial && grads && live_idx && live_cnt, "null pointer");
  return bwd_launch(kind, n, S, draw, act, params, packed_bwd, dact, partial, grads, live_idx, live_cnt, stream, MM_X6);
}
