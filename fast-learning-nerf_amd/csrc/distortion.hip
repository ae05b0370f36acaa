// distortion.hip -- the distortion loss of mip-NeRF 360 on the weights of a ray, and its gradient in the weights (gfx950).
//
//   l = sum_i sum_j w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 delta_i
// over the S intervals [e_i, e_{i+1}] of a ray, e_i = z_i, e_S = max(far, z_{S-1}), with m_i / delta_i the midpoint / width of the
// interval after the normalisation t(x) of the sampler (linear in depth, or in disparity with lindisp); include/fastnerf.h has the contract.
//
// Mapping: composite.hip's -- ONE 64-lane wavefront per ray, lane l owns the C = ceil(S/64) consecutive samples l*C .. l*C + C-1, the
// sums along the ray are wave-level shuffle scans (no LDS round trip, no barrier, no atomics: bit-identical from run to run).
//
// Order of the arithmetic.  The textbook O(S) form m_i W_{<i} - WM_{<i} subtracts two prefix sums of order 1 to get a number of order
// |m_i - m_j|: samples clustered within 1e-3 of a surface lose three digits (what composite.hip says of `total - inclusive prefix`).
// Here nothing cancels.  With gamma_k = m_{k+1} - m_k >= 0 taken from the DEPTH difference e_{k+2} - e_k (never from two t values),
//   |m_i - m_j| = sum_{min(i,j) <= k < max(i,j)} gamma_k
//   sum_j w_j |m_i - m_j| = A_i + B_i,   A_i = sum_{k<i} gamma_k P_k,   B_i = sum_{k>=i} gamma_k Q_k
//   P_k = sum_{j<=k} w_j (from the near end),   Q_k = sum_{j>k} w_j (from the far end)
//   dl/dw_i = 2 (A_i + B_i) + 2/3 w_i delta_i,    l = 2 sum_i w_i A_i + 1/3 sum_i w_i^2 delta_i
// every summand is non-negative: two nested sums of at most S terms, relative error of the order of S 2^-24 whatever the depths are.
#include "common.h"

#define WAVE 64
#define MAXC 8  // up to 512 samples per ray

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
  return v;
}

// p -> the sum of the lanes BELOW this one, added from the near end; q -> the sum of the lanes ABOVE it, added from the far end.  Two
// independent scans, interleaved so that their cross-lane latencies overlap.
__device__ __forceinline__ void wave_prefix_suffix_add(float& p, float& q, int lane) {
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    const float tp = __shfl_up(p, o, WAVE), tq = __shfl_down(q, o, WAVE);
    if (lane >= o) p += tp;
    if (lane + o < WAVE) q += tq;
  }
  const float below = __shfl_up(p, 1, WAVE), above = __shfl_down(q, 1, WAVE);
  p = lane == 0 ? 0.0f : below;
  q = lane == WAVE - 1 ? 0.0f : above;
}

__global__ void __launch_bounds__(256) distortion_kernel(int64_t n, int S, const float* __restrict__ w, const float* __restrict__ z,
                                                          const float* __restrict__ rays, int lindisp,
                                                          const uint8_t* __restrict__ skip, float coef,
                                                          const float* __restrict__ g_up, float* __restrict__ ell,
                                                          float* __restrict__ g_w) {
  const int lane = threadIdx.x & 63;
  const int C = (S + WAVE - 1) / WAVE;
  const int s0 = lane * C;
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t r = wave0; r < n; r += nwaves) {
    const float near = rays[r * 11 + 6], far = rays[r * 11 + 7];
    // 1 / (t's denominator): the depth span, or the disparity span with lindisp
    const float span = lindisp ? 1.0f / near - 1.0f / far : far - near;
    const bool live = span > 0.0f && span < __builtin_huge_valf() && !(skip && skip[r]);   // (wave-uniform; a NaN span is not > 0)
    if (!live) {
      if (ell && lane == 0) ell[r] = 0.0f;
      if (g_w) {
#pragma unroll
        for (int j = 0; j < MAXC; ++j)
          if (j < C && s0 + j < S) g_w[r * S + s0 + j] = 0.0f;
      }
      continue;
    }
    const float inv = 1.0f / span;
    const float* zr = z + r * S;
    const float* wr = w + r * S;
    const float e_end = fmaxf(far, zr[S - 1]);
    // the chunk's edges e[0 .. cnt+1] (edge S is e_end; the one behind it is never used: gamma_{S-1} has no interval to reach)
    float e[MAXC + 2], wj[MAXC], gam[MAXC], del[MAXC];
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < MAXC + 2; ++j) {
      if (j >= C + 2) break;
      const int s = s0 + j;
      e[j] = s < S ? zr[s] : e_end;
    }
    float cw = 0.0f;
#pragma unroll
    for (int j = 0; j < MAXC; ++j) {
      if (j >= C) break;
      const int s = s0 + j;
      if (s >= S) break;
      wj[j] = wr[s];
      const float d1 = e[j + 1] - e[j], d2 = e[j + 2] - e[j];
      if (lindisp) {
        del[j] = d1 / (e[j] * e[j + 1]) * inv;
        gam[j] = s + 1 < S ? 0.5f * d2 / (e[j] * e[j + 2]) * inv : 0.0f;
      } else {
        del[j] = d1 * inv;
        gam[j] = s + 1 < S ? 0.5f * d2 * inv : 0.0f;
      }
      cw += wj[j];
      cnt = j + 1;
    }
    // P (inclusive, from the near end) and Q (exclusive, from the far end) of the weights
    float pre = cw, suf = cw;
    wave_prefix_suffix_add(pre, suf, lane);
    float gp[MAXC], gq[MAXC];
    float cgp = 0.0f, cgq = 0.0f;
#pragma unroll
    for (int j = 0; j < MAXC; ++j) {
      if (j < cnt) {
        pre += wj[j];
        gp[j] = gam[j] * pre;
        cgp += gp[j];
      }
    }
#pragma unroll
    for (int j = MAXC - 1; j >= 0; --j) {
      if (j < cnt) {
        gq[j] = gam[j] * suf;
        cgq += gq[j];
        suf += wj[j];
      }
    }
    // A (exclusive, from the near end) and B (inclusive, from the far end)
    float a = cgp, b = cgq;
    wave_prefix_suffix_add(a, b, lane);
    float Bj[MAXC];
#pragma unroll
    for (int j = MAXC - 1; j >= 0; --j) {
      if (j < cnt) {
        b += gq[j];
        Bj[j] = b;
      }
    }
    const float c = g_w ? coef * (g_up ? g_up[r] : 1.0f) : 0.0f;
    float lsum = 0.0f;
#pragma unroll
    for (int j = 0; j < MAXC; ++j) {
      if (j < cnt) {
        const float wd = wj[j] * del[j];
        // (+ 0.0f: a zero gradient is +0 under a negative coef too)
        if (g_w) g_w[r * S + s0 + j] = c * (2.0f * (a + Bj[j]) + (2.0f / 3.0f) * wd) + 0.0f;
        lsum += 2.0f * (wj[j] * a) + (1.0f / 3.0f) * (wj[j] * wd);
        a += gp[j];
      }
    }
    if (ell) {
      lsum = wave_sum(lsum);
      if (lane == 0) ell[r] = lsum;
    }
  }
}

static inline int grid_waves(int64_t n) {
  int64_t g = (n + 3) / 4;  // 4 waves (rays) per 256-thread block
  if (g < 1) g = 1;
  if (g > 4096) g = 4096;
  return (int)g;
}

extern "C" int fastnerf_distortion(int64_t n, int S, const float* w, const float* z, const float* rays11, int lindisp,
                                   const uint8_t* skip, float coef, const float* g_up, float* ell, float* g_w, fn_stream_t stream) {
  FN_CHECK_ARG(n >= 0 && S >= 1 && S <= WAVE * MAXC, "n>=0, 1<=S<=512");
  FN_CHECK_ARG(n == 0 || (w && z && rays11 && (ell || g_w)), "null pointer");
  if (n == 0) return 0;
  hipLaunchKernelGGL(distortion_kernel, dim3(grid_waves(n)), dim3(256), 0, fn::S(stream), n, S, w, z, rays11, lindisp ? 1 : 0, skip,
                     coef, g_up, ell, g_w);
  FN_LAUNCH_CHECK();
  return 0;
}
