// mlp_bwd_dx.hip -- the dY chain of the backward pass: one persistent kernel walks the layers in reverse with transposed packed weights and
// leaves every layer's pre-activation gradient in HBM for the dW jobs (mlp_bwd_dw.hip launches it through fn_launch_dx).
#include "mlp_common.h"
#include "dw_pair.h"   // FN_DX_NO_DYV_STORE

// =========================================================================================
// backward: dX chain
// =========================================================================================
// epilogue: optional rank-1 term (dalpha x wa), ReLU mask from the forward's ballot words, write H
// and the pre-activation gradient buffer.
struct DxPre {  // loaded before the k-loop (see load_bias)
  unsigned mlo, mhi;
  float wan[4];   // rank-1 weights of this lane's columns: two column tiles of 32, or four of 16 (L16)
};
template <bool MASK, bool RANK1, bool L16 = false>
__device__ __forceinline__ DxPre dx_preload(const unsigned long long* __restrict__ maskw, const float* __restrict__ wa,
                                            int wn, int lane) {
  DxPre p;
  p.mlo = p.mhi = 0u;
  p.wan[0] = p.wan[1] = p.wan[2] = p.wan[3] = 0.f;
  if (MASK) {
    const unsigned long long w = maskw[lane];
    p.mlo = (unsigned)w;
    p.mhi = (unsigned)(w >> 32);
  }
  if (RANK1) {
    if constexpr (L16) {
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) p.wan[ct] = wa[(wn * 4 + ct) * 16 + (lane & 15)];
    } else {
      p.wan[0] = wa[(wn * 2 + 0) * 32 + (lane & 31)];
      p.wan[1] = wa[(wn * 2 + 1) * 32 + (lane & 31)];
    }
  }
  return p;
}
template <bool MASK, bool RANK1>
__device__ __forceinline__ void epilogue_dx(const f32x4m (&acc)[4][4], float* Hs, const float* Es_dalpha, const DxPre& pre,
                                            float* __restrict__ dsave, int wm, int wn, int lane, int valid) {
  asm volatile("" : "+v"(lane));
  const unsigned mlo = pre.mlo, mhi = pre.mhi;
  float* colp[4][4];
  h_cols16<4>(Hs, wm, wn, lane, colp);
  const int hq = lane >> 4;
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const float wan = pre.wan[ct];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[mt][ct][r];
        if (RANK1) v = fmaf(Es_dalpha[wm * 64 + mt * 16 + 4 * hq + r], wan, v);
        if (MASK) {   // this lane's sign word of the forward (epilogue_fwd, same enumeration)
          const int idx = (mt * 4 + ct) * 4 + r;
          const int keep = __builtin_amdgcn_sbfe(idx < 32 ? (int)mlo : (int)mhi, 31 - (idx & 31), 1);
          v = __int_as_float(__float_as_int(v) & keep);
        }
        H16_AT(colp, ct, mt, r) = v;
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <bool MASK, bool RANK1>
__device__ __forceinline__ void epilogue_dx(const f32x16 (&acc)[2][2], float* Hs, const float* Es_dalpha,
                                            const DxPre& pre, float* __restrict__ dsave, int wm, int wn, int lane,
                                            int valid) {
  asm volatile("" : "+v"(lane));
  const unsigned mlo = pre.mlo, mhi = pre.mhi;
  float* colp[2][8];
  h_cols<2>(Hs, wm, wn, lane, colp);
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int n = (wn * 2 + nt) * 32 + (lane & 31);
    const float wan = pre.wan[nt];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = wm * 64 + mt * 32 + crow(r, lane);
        float v = acc[mt][nt][r];
        if (RANK1) v = fmaf(Es_dalpha[m], wan, v);
        if (MASK) {   // this lane's sign word of the forward (epilogue_fwd): value idx is bit 31 - (idx & 31) of half idx >> 5
          const int idx = (nt * 2 + mt) * 16 + r;
          const int keep = __builtin_amdgcn_sbfe(idx < 32 ? (int)mlo : (int)mhi, 31 - (idx & 31), 1);   // 0 or -1
          v = __int_as_float(__float_as_int(v) & keep);
        }
        H_AT(colp, nt, mt, r) = v;
        if (dsave != nullptr && m < valid) dsave[(unsigned)(m * 256 + n)] = v;
      }
      __builtin_amdgcn_sched_barrier(0);  // bound live ranges: one 32x32 tile at a time
    }
  }
}

template <int MM = MM_F32>
__global__ void __launch_bounds__(NTHR, 2 * NTHR / 512 * WG_PER_CU)
mlp_bwd_dx_kernel(int64_t P, const float* __restrict__ draw, const float* __restrict__ act,
                  const float* __restrict__ params, const float* __restrict__ packed_t, float* __restrict__ dact,
                  NetLayout lay, unsigned* __restrict__ sched, const int* __restrict__ live_idx,
                  const int* __restrict__ live_cnt, float* __restrict__ headws, int flags) {
  const int64_t PL = P;   // (live-list mode: see the forward kernel)
  if (live_idx) P = (int64_t)__builtin_amdgcn_readfirstlane(*live_cnt);
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Hs = smem;
  float* Es = smem + LDS_H;  // Es[0..127] = dalpha of the tile's rows; headws: Es[128 + c * TM + m] = draw[m][c], c = 0..2 (the head-gradient block below)
  volatile int* sched_word = reinterpret_cast<volatile int*>(Es + 1024);   // tile scheduler word (sched.h): unused part of Es
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int64_t ntiles = (P + TM - 1) / TM;
  stagger_start();

  for (int64_t tile = blockIdx.x; tile < ntiles;) {
    const int64_t p0 = tile * TM;
    const int valid = (int)((P - p0) < TM ? (P - p0) : TM);
    const unsigned long long* maskw =
        reinterpret_cast<const unsigned long long*>(act + act_mask(PL, lay.pe_pad)) + tile * (8 * NWAVES * 64);
    // ---- phase A: dYv = (drgb . Wr) * [hv > 0] -> H[:, 0:128] --------------------------
    {
      const int pm = tid >> 2, pq = tid & 3;
      const bool ok = pm < valid;
      const bool keep = ok && !(flags & FN_DX_NO_DYV_STORE);   // (the view job rebuilds dYv from hv, draw and Wr: dw_pair.h)
      const int64_t pp = ok ? p0 + pm : P - 1;
      const float4 dr = *reinterpret_cast<const float4*>(draw + (live_idx ? (int64_t)live_idx[pp] : pp) * 4);
      if (pq == 0) Es[pm] = ok ? dr.w : 0.f;
      if (pq < 3) Es[128 + pq * TM + pm] = ok ? (pq == 0 ? dr.x : pq == 1 ? dr.y : dr.z) : 0.f;   // (stored with or without headws, like hv below: no branch in this phase)
      const float* wr = params + lay.RW;
      asm volatile("" : "+s"(wr));   // per tile: hoisted out of the tile loop, the 96 registers of Wr are spilled to scratch
      const float* hv = act + act_hv(PL, lay.pe_pad) + pp * 128;
      float* dyv = dact + dact_yv(PL) + pp * 128;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int k = pq * 32 + i * 4;
        const float4 h = *reinterpret_cast<const float4*>(hv + k);
        const float4 w0 = *reinterpret_cast<const float4*>(wr + k);
        const float4 w1 = *reinterpret_cast<const float4*>(wr + 128 + k);
        const float4 w2 = *reinterpret_cast<const float4*>(wr + 256 + k);
        float4 o;
        o.x = dyv_value(h.x, dr.x, dr.y, dr.z, w0.x, w1.x, w2.x);
        o.y = dyv_value(h.y, dr.x, dr.y, dr.z, w0.y, w1.y, w2.y);
        o.z = dyv_value(h.z, dr.x, dr.y, dr.z, w0.z, w1.z, w2.z);
        o.w = dyv_value(h.w, dr.x, dr.y, dr.z, w0.w, w1.w, w2.w);
        if (!ok) o = make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(Hs + pm * 256 + ((((k >> 2) ^ (pm & 15))) << 2)) = o;
        if (keep) store_nt(dyv + k, o);
        // hv itself into the half of H that phase A leaves free (columns 128 + k, same swizzle): the head gradients below
        *reinterpret_cast<float4*>(Hs + pm * 256 + ((32 + ((k >> 2) ^ (pm & 15))) << 2)) = ok ? h : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    __syncthreads();
    // ---- rgb head + alpha bias gradients of this tile (what head_grads_kernel takes a second pass over hv and draw for) ----
    // headws[tile][0..383] = dWr[c][k] = sum_m draw[m][c] hv[m][k], [384..386] = dbr[c], [387] = dba: one thread per output (threads
    // 0..127: channels 0 and 2 of column tid, which share the hv reads; 128..255: channel 1 of column tid - 128; 128..131 also the four plain sums), each a
    // sum over the tile's rows in ascending order -- the value depends on the tile's points alone.  Rows >= valid hold zeros.
    if (headws != nullptr) {
      float* const o = headws + tile * 388;
      int ht = tid;
      asm volatile("" : "+v"(ht));   // this block's addresses are formed per tile: as loop invariants they cost registers the products need
      const int k = ht & 127;
      const float* hc = Hs + ((32 + (k >> 2)) << 2) + (k & 3);   // column 128 + k of row 0, before the swizzle
      const int sw = (k >> 2) & 15;
      const float* da = Es + 128 + (wave >> 1) * TM;             // channel 0 (waves 0, 1) / channel 1 (waves 2, 3)
      const float* dc = Es + 128 + 2 * TM;
      float s0 = 0.f, s2 = 0.f;   // (waves 2, 3 form s2 as well and drop it: one loop for the workgroup)
#pragma unroll 1
      for (int m0 = 0; m0 < TM; m0 += 16) {   // 16 rows at a time: the swizzle is a compile-time offset, the registers stay few
        float h[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) h[j] = hc[(m0 + j) * 256 + ((sw ^ j) - sw) * 4];
#pragma unroll
        for (int j = 0; j < 16; j += 4) {
          const float4 a = *reinterpret_cast<const float4*>(da + m0 + j);
          const float4 c = *reinterpret_cast<const float4*>(dc + m0 + j);
          s0 = fmaf(a.x, h[j], s0);     s2 = fmaf(c.x, h[j], s2);
          s0 = fmaf(a.y, h[j + 1], s0); s2 = fmaf(c.y, h[j + 1], s2);
          s0 = fmaf(a.z, h[j + 2], s0); s2 = fmaf(c.z, h[j + 2], s2);
          s0 = fmaf(a.w, h[j + 3], s0); s2 = fmaf(c.w, h[j + 3], s2);
        }
      }
      o[(wave >> 1) * 128 + k] = s0;
      if (wave < 2) o[256 + k] = s2;
      if (ht >= 128 && ht < 132) {   // dbr[0..2], dba
        const float* ds = ht == 131 ? Es : Es + 128 + (ht - 128) * TM;
        float sb = 0.f;
#pragma unroll 1
        for (int m = 0; m < TM; m += 4) {
          const float4 a = *reinterpret_cast<const float4*>(ds + m);
          sb += a.x; sb += a.y; sb += a.z; sb += a.w;
        }
        o[256 + ht] = sb;
      }
    }
    constexpr bool L16 = MM != MM_F32;
    // every 256 x 256 product after the first finds its first weights loaded one layer ahead (gemm_seg16, "chained weights")
    constexpr bool CHAIN = L16;
    AccT<L16, 2> acc;
    WRegsT<L16, 2> wch;
    // ---- dY7 = (dYv . M + dalpha x wa) * [h7 > 0]  (K = 128; M = Wv[:, :256] Wf, the folded view layer: mlp_pack.hip) ----
    zero_acc<2>(acc);
    {
      const DxPre pre = dx_preload<true, true, L16>(maskw + (7 * NWAVES + wave) * 64, params + lay.AW, wn, lane);
      gemm<MM, 2, 0>(acc, Hs, 0, 16, wblock<MM>(packed_t, lay.PBM), 16, 0, wn * 2, wm, lane);
      __syncthreads();
      wprefetch(wch, wblock<MM>(packed_t, lay.PB[2]), 32, 0, 32, wn * 2, lane);
      epilogue_dx<true, true>(acc, Hs, Es, pre, nullptr, wm, wn, lane, valid);
    }
    __syncthreads();
    // ---- dY_{l-1} = (dY_l . W_l) * [h_{l-1} > 0],  l = 7..1 ------------------------------
#pragma unroll 1
    for (int l = 7; l >= 1; --l) {
      const int64_t off = lay.PB[9 - l];   // PB[2] = L7t ... PB[8] = L1t
      zero_acc<2>(acc);
      const DxPre pre = dx_preload<true, false, L16>(maskw + ((l - 1) * NWAVES + wave) * 64, nullptr, wn, lane);
      gemm<MM, 2, 0, CHAIN>(acc, Hs, 0, 32, wblock<MM>(packed_t, off), 32, 0, wn * 2, wm, lane, 0,
                            dact + dact_y(PL, l) + p0 * 256, valid, wave, wch);    // streams dY_l (what it reads) out
      __syncthreads();
      wprefetch(wch, wblock<MM>(packed_t, lay.PB[l > 1 ? 10 - l : 8]), 32, 0, 32, wn * 2, lane);   // (l == 1: nobody's; a re-read)
      epilogue_dx<true, false>(acc, Hs, Es, pre, nullptr, wm, wn, lane, valid);
      __syncthreads();
    }
    {   // dY0 has no consumer loop: copy it out row-wise
      float* d0 = dact + dact_y(PL, 0) + p0 * 256;
      for (int i = tid; i < TM * 64; i += NTHR) {
        const int m = i >> 6, sl = i & 63;
        if (m < valid)
          store_nt(d0 + m * 256 + ((sl ^ (m & 15)) << 2), *reinterpret_cast<const float4*>(Hs + m * 256 + sl * 4));
      }
    }
    tile = b_next_tile(sched, sched_word, tid);   // closing barrier inside: H is rewritten by the next tile's phase A
  }
  b_sched_exit(sched, tid);
}

template <int MM>
static int launch_dx_t(int grid, hipStream_t st, int64_t P, const float* draw, const float* act, const float* params, const float* packed_bwd,
                       float* dact, const NetLayout& L, const int* live_idx, const int* live_cnt, float* headws, int flags) {
  static fn::DevOnce once;
  if (int rc = fn::set_dyn_lds(reinterpret_cast<const void*>(&mlp_bwd_dx_kernel<MM>), once, LDS_BYTES)) return rc;
  unsigned* sched = b_sched_pair();
  FN_CHECK_ARG(sched != nullptr, "scheduler counters (hipMalloc failed?)");
  hipLaunchKernelGGL(mlp_bwd_dx_kernel<MM>, dim3(grid), dim3(NTHR), LDS_BYTES, st, P, draw, act, params, packed_bwd, dact, L, sched, live_idx, live_cnt, headws, flags);
  FN_LAUNCH_CHECK();
  return 0;
}
// headws: room for [ceil(P / TM)][388] per-tile rgb-head / alpha-bias partials (P the capacity in live-list mode), or nullptr: not formed
// flags: 0, or FN_DX_NO_DYV_STORE
int fn_launch_dx(int mm, int grid, hipStream_t st, int64_t P, const float* draw, const float* act, const float* params, const float* packed_bwd,
                 float* dact, const NetLayout& L, const int* live_idx, const int* live_cnt, float* headws, int flags) {
  return mm == MM_X6 ? launch_dx_t<MM_X6>(grid, st, P, draw, act, params, packed_bwd, dact, L, live_idx, live_cnt, headws, flags)
                     : launch_dx_t<MM_F32>(grid, st, P, draw, act, params, packed_bwd, dact, L, live_idx, live_cnt, headws, flags);
}
// The chain alone, on the grid the backward entry points give it (mlp_bwd_dw.hip, bwd_launch_t): for a caller that wants the
// pre-activation gradients and no dW (sigma_grad.hip).
int fn_launch_dx_alone(int mm, int kind, int64_t P, const float* draw, const float* act, const float* params, const float* packed_bwd,
                       float* dact, hipStream_t st) {
  const int64_t ntiles = (P + TM - 1) / TM;
  int grid = fn::device_cus() * WG_PER_CU;
  if (ntiles < grid) grid = (int)ntiles;
  return fn_launch_dx(mm, grid, st, P, draw, act, params, packed_bwd, dact, layout_of(kind), nullptr, nullptr, nullptr, 0);
}
