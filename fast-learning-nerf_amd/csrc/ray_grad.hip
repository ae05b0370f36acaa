// ray_grad.hip -- d(loss)/d(ray): the gradient of one pass of render_rays with respect to its ray batch [n, 11] = (o, d, near, far,
// viewdir), for pose refinement and view registration through the fused renderer (render.py _RenderRaysRayGradFn).
//
// Contract of fastnerf_ray_grad (include/fastnerf.h): called AFTER the MLP backward of a pass (fastnerf_mlp_bwd_ex / _x6_bwd on
// draw = d(loss)/d(raw) from fastnerf_raw2outputs_bwd), while that pass's `dact` and `act` are still what the backward left.  It enqueues
//   1. sigma_grad_kernel (sigma_grad.hip, through fn_launch_sigma_grad: the same kernel, not a copy) on the caller's dY0 / dY5 / pe.
//      With the cotangent of a real loss in dact it yields g[p] = d(loss)/d(point p) into `ws` [P, 3];
//   2. ray_grad_kernel below, which folds g, the compositing's dependence on |d| and the view-direction branch into d_rays [n, 11].
//
// What it differentiates (render.py:195-305 as autograd sees it; z is a constant of the pass: the coarse z depends on near / far only,
// the fine z_samples are detached at render.py:281):
//   point p = o + d z           =>  d_o[r] = sum_s g[r,s],   d_d[r] = sum_s z[r,s] g[r,s] + (the dists term)
//   dists = dz |d| (render.py:167), alpha = 1 - exp(-relu(sigma') dist), sigma' = raw[..., 3] + noise:
//       dL/d(dist) = dL/d(sigma') sigma' / dist  and  dist = dz |d|   =>   dL/d|d| = sum_s draw[r,s,3] sigma'[r,s] / |d|,
//       with no division by dist: a sample with dz = 0 or sigma' <= 0 has draw[..., 3] = 0 and contributes an exact 0, and so does the
//       last sample (1e10 |d|: exp(..) = 0).  d|d|/dd = d / |d|   =>   the dists term is c_r d_r / |d_r|^2, c_r = sum_s draw[r,s,3] sigma'[r,s].
//       (|d|^2 summed as compositing sums it; exactly 0 for a ray with d = 0, where torch's norm has the subgradient 0.)
//   view layer: zv = M h7 + Wv[:, 256:283] vpe + b', vpe = PE(4) of the ray's viewdir, the same for every sample of the ray, so
//       dvpe[c] = sum_j (sum_s dYv[r,s,j]) Wv[j][256 + c]   (one [128] x [128 x 27] product per ray),
//       d_v[a]  = dvpe[a] + sum_k 2^k (dvpe[sin_k,a] vpe[cos_k,a] - dvpe[cos_k,a] vpe[sin_k,a])     k = 0..3, the SAVED sines / cosines of sample 0.
//   near / far (columns 6:8) are constants of this gradient: exact zeros.
//
// ray_grad_kernel: one workgroup of four waves per ray, any grid order (a ray's result depends on its own rows only).
//   * Bound: HBM.  Per sample it reads 512 B of dYv, 12 B of g and 36 B of z / draw / raw (+ 4 B of noise when given) against 128 + 7
//     adds: 560 B at 6.3 TB/s is 0.09 ns per sample, no arithmetic comes near that.  Together with sigma_grad_kernel (2 KiB of
//     dY0 / dY5 + 256 B of pe + 12 B of g written, sigma_grad.hip header) a pass moves 2.9 KB per sample: 0.46 ns.  The 128 x 27 weights
//     (14 KB) stay in L2.  Measured: profiles/ray_grad.md.
//   * dYv: whole 512-byte rows, 16 bytes per lane, 8 rows per workgroup iteration (slot q = tid / 32 takes samples q, q + 8, ...); draw and
//     raw are read as whole float4 rows, z / noise / g as consecutive floats of consecutive lanes (g rows are 12 bytes: a ray's first
//     one is 16-byte aligned only when S is a multiple of 4).
//   * Summation order, fixed, no atomics: per slot (dYv) or per thread (the seven per-sample sums: thread t takes samples t, t + 256, ...)
//     samples ASCENDING; then dYv slots 0..7 ascending, the per-sample sums over the xor-butterfly 32, 16, .., 1 of a wave and waves 0..3
//     ascending; the 128 products of a dvpe column as channels 0..63 and 64..127 ascending, the first half plus the second; the four
//     frequency terms ascending.  Every product and sum is rounded on its own.  Two calls agree bit for bit, wherever the ray sits in
//     the batch.
//   * accumulate != 0 adds to what d_rays holds (the second pass of a render adds to the first); 0 overwrites all 11 columns.
//     Nothing is read or written past row n - 1.
#include "common.h"
#include "mlp_layout.h"

using namespace fnl;

#define RG_THREADS 256
#define RG_SLOTS 8      // dYv rows in flight per workgroup iteration (RG_THREADS / 32)

__global__ void __launch_bounds__(RG_THREADS)
ray_grad_kernel(int S, const float* __restrict__ rays, const float* __restrict__ z, const float* __restrict__ raw,
                const float* __restrict__ noise, const float* __restrict__ draw, const float* __restrict__ g,
                const float* __restrict__ dyv, const float* __restrict__ vpe, const float* __restrict__ Wv, int accumulate,
                float* __restrict__ d_rays) {
  __shared__ __attribute__((aligned(16))) float Ys[RG_SLOTS * 128];
  __shared__ float Rs[4 * 8];
  __shared__ float Vs[32];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int64_t r = blockIdx.x;
  const int64_t p0 = r * S;

  // sum over the ray's samples of dYv [S, 128]: slot q, columns 4 cg .. 4 cg + 3
  {
    const int q = tid >> 5, cg = tid & 31;
    const float* src = dyv + p0 * 128 + cg * 4;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s = q; s < S; s += RG_SLOTS) {
      const float4 v = *reinterpret_cast<const float4*>(src + (int64_t)s * 128);
      a.x = fadd(a.x, v.x); a.y = fadd(a.y, v.y); a.z = fadd(a.z, v.z); a.w = fadd(a.w, v.w);
    }
    *reinterpret_cast<float4*>(Ys + q * 128 + cg * 4) = a;
  }
  // the seven per-sample sums: g (3), z g (3), draw[..., 3] sigma'
  float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int s = tid; s < S; s += RG_THREADS) {
    const int64_t p = p0 + s;
    const float gx = g[p * 3], gy = g[p * 3 + 1], gz = g[p * 3 + 2];
    const float zz = z[p];
    const float4 dr = *reinterpret_cast<const float4*>(draw + p * 4);
    const float4 rw = *reinterpret_cast<const float4*>(raw + p * 4);
    float sig = rw.w;
    if (noise) sig = fadd(sig, noise[p]);
    acc[0] = fadd(acc[0], gx); acc[1] = fadd(acc[1], gy); acc[2] = fadd(acc[2], gz);
    acc[3] = fadd(acc[3], fmul(zz, gx)); acc[4] = fadd(acc[4], fmul(zz, gy)); acc[5] = fadd(acc[5], fmul(zz, gz));
    acc[6] = fadd(acc[6], fmul(dr.w, sig));
  }
#pragma unroll
  for (int i = 0; i < 7; ++i) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc[i] = fadd(acc[i], __shfl_xor(acc[i], off, 64));
    if (lane == 0) Rs[wave * 8 + i] = acc[i];
  }
  __syncthreads();
  // slots 0..7 ascending; column tid of every slot is read by thread tid alone, so the total may replace slot 0's
  if (tid < 128) {
    float y = Ys[tid];
#pragma unroll
    for (int q = 1; q < RG_SLOTS; ++q) y = fadd(y, Ys[q * 128 + tid]);
    Ys[tid] = y;
  }
  __syncthreads();
  // dvpe[c] = sum_j Ys[j] Wv[j][256 + c]: lanes (c, half) of wave 0, channels 64 half .. 64 half + 63
  if (tid < 64) {
    const int c = tid & 31, half = tid >> 5;
    float d = 0.f;
    if (c < 27) {
      const float* w = Wv + (int64_t)(half * 64) * 283 + 256 + c;
      const float* y = Ys + half * 64;
#pragma unroll 8
      for (int j = 0; j < 64; ++j) d = fadd(d, fmul(y[j], w[j * 283]));
    }
    d = fadd(d, __shfl_xor(d, 32, 64));
    if (tid < 32) Vs[tid] = d;      // columns 27..31: zeros
  }
  __syncthreads();
  if (tid >= 11) return;
  float val = 0.f;
  if (tid < 6) {
    const int a = tid < 3 ? tid : tid - 3;
    const int i = tid;      // Rs column: g for o, z g for d
    val = fadd(fadd(fadd(Rs[i], Rs[8 + i]), Rs[16 + i]), Rs[24 + i]);
    if (tid >= 3) {
      const float* rr = rays + r * 11;
      const float c = fadd(fadd(fadd(Rs[6], Rs[8 + 6]), Rs[16 + 6]), Rs[24 + 6]);
      const float dd = fadd(fadd(fmul(rr[3], rr[3]), fmul(rr[4], rr[4])), fmul(rr[5], rr[5]));
      if (dd > 0.f) val = fadd(val, fmul(c, rr[3 + a]) / dd);
    }
  } else if (tid >= 8) {
    const int a = tid - 8;
    const float* e = vpe + p0 * 32;
    val = Vs[a];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int cs = 3 + 6 * k + a, cc = 6 + 6 * k + a;
      val = fadd(val, fmul((float)(1 << k), fsub(fmul(Vs[cs], e[cc]), fmul(Vs[cc], e[cs]))));
    }
  }
  float* out = d_rays + r * 11 + tid;
  *out = accumulate ? fadd(*out, val) : val;
}

static inline int64_t up4(int64_t v) { return (v + 3) / 4 * 4; }

// g [n*S, 3]
extern "C" int64_t fastnerf_ray_grad_ws_floats(int math_mode, int64_t n, int S) {
  if (math_mode < 0 || math_mode > 2 || n < 0 || S < 1) {
    fn::set_error("fastnerf_ray_grad_ws_floats: bad argument: math_mode in {0,1,2}, n>=0, S>=1");
    return -1;
  }
  return up4(3 * n * S);
}

extern "C" int fastnerf_ray_grad(int math_mode, int kind, int64_t n, int S, const float* rays11, const float* z, const float* raw,
                                 const float* noise, const float* draw, const float* act, const float* dact, const float* params,
                                 float* ws, int accumulate, float* d_rays, fn_stream_t stream) {
  FN_CHECK_ARG(math_mode >= 0 && math_mode <= 2 && n >= 0 && n <= 0x7fffffff && S >= 1, "math_mode in {0,1,2}, 0<=n<2^31, S>=1");
  if (kind != 0) {
    fn::set_error("fastnerf_ray_grad: kind %d is not supported: the ray gradient exists for kind 0 (NeRF) only", kind);
    return -1;
  }
  if (math_mode == 1) {
    fn::set_error("fastnerf_ray_grad: math mode 1 (bf16x3) is not supported: its K-fragment tensors have no ray-gradient kernel; "
                  "use math mode 0 (fp32) or 2 (bf16x6)");
    return -1;
  }
  FN_CHECK_ARG(n == 0 || (rays11 && z && raw && draw && act && dact && params && ws && d_rays), "null pointer");
  if (n == 0) return 0;
  const int64_t P = n * S;
  hipStream_t st = fn::S(stream);
  if (int rc = fn_launch_sigma_grad(math_mode, P, act, dact, nullptr, params, nullptr, ws, st)) return rc;
  const NetLayout L = make_layout(0);
  hipLaunchKernelGGL(ray_grad_kernel, dim3((unsigned)n), dim3(RG_THREADS), 0, st, S, rays11, z, raw, noise, draw,
                     static_cast<const float*>(ws), dact + dact_yv(P), act + act_vpe(P, L.pe_pad), params + L.VW, accumulate,
                     d_rays);
  FN_LAUNCH_CHECK();
  return 0;
}
