// pose.hip -- a table of camera poses that training refines, for gfx950: the exponential map of a per-image 6-vector onto its base
// pose, its backward, and the reduction of a ray batch's gradient to one 3x4 gradient per image (include/fastnerf.h, "pose table").
//
//   R_i = exp(hat(omega_i)) R0_i,  t_i = t0_i + tau_i      (the camera turns about its own centre, in world axes)
//   o = t,  d = R dir,  v = d / |d|,  dir = ((col - cx) / fx, -(row - cy) / fy, -1)      (pinhole.h, pack_rays_kernel of rays.hip)
//
// Every sum and product whose order matters goes through fadd / fmul / fsub (common.h): nothing is contracted.  The two exp kernels run
// one lane per image; pose_grad is the one with work in it, a segmented sum without atomics.
#include "common.h"
#include "pinhole.h"
#include "seg_reduce.h"

// Rodrigues' coefficients of theta^2 = |omega|^2, each in a form in which nothing cancels and nothing divides by zero:
//   a = sin(theta) / theta,   b = (1 - cos(theta)) / theta^2 = 1/2 (sin(theta/2) / (theta/2))^2,   c = (theta - sin(theta)) / theta^3
// a and b by series below theta = 1e-3 (the first dropped term is theta^6 / 5040 < 2e-22), so a(0) = 1 and b(0) = 1/2 exactly.
// c's difference loses log2(6 / theta^2) bits: it is taken by series below theta = 0.5 (first dropped term theta^8 / 39916800 < 1e-10),
// and above it the difference keeps all but 5 bits of a coefficient that multiplies K^2 = O(theta^2).
#define FN_POSE_SERIES_AB 1e-3f
#define FN_POSE_SERIES_C 0.5f

__device__ __forceinline__ float sinc_f(float x, float x2) {      // sin(x) / x
  if (x < FN_POSE_SERIES_AB) return fadd(fsub(1.0f, fmul(x2, 1.0f / 6.0f)), fmul(fmul(x2, x2), 1.0f / 120.0f));
  return sinf(x) / x;
}

struct Rodrigues {
  float a, b, c;
};

__device__ __forceinline__ Rodrigues rodrigues(float th2, bool want_c) {
  Rodrigues r;
  const float th = sqrtf(th2);
  r.a = sinc_f(th, th2);
  const float sh = sinc_f(fmul(0.5f, th), fmul(0.25f, th2));
  r.b = fmul(0.5f, fmul(sh, sh));
  r.c = 0.0f;
  if (want_c) {
    if (th < FN_POSE_SERIES_C) {      // 1/6 - x/120 + x^2/5040 - x^3/362880, x = theta^2 (Horner)
      float s = fsub(1.0f / 5040.0f, fmul(th2, 1.0f / 362880.0f));
      s = fsub(1.0f / 120.0f, fmul(th2, s));
      r.c = fsub(1.0f / 6.0f, fmul(th2, s));
    } else {
      r.c = fsub(th, sinf(th)) / fmul(th2, th);
    }
  }
  return r;
}

// A = exp(hat(w)) R0 into a[9] (row-major); R0 = the rotation of the row-major 3x4 base pose.  th2 == 0 (w = 0, or so small that its
// square underflows: the rotation is the identity to 1e-22): the base's own bits.
__device__ __forceinline__ void compose(const float w[3], float th2, const Rodrigues& r, const float* __restrict__ base, float a[9]) {
  if (th2 == 0.0f) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int k = 0; k < 3; ++k) a[3 * j + k] = base[4 * j + k];
    return;
  }
  // R = I + a K + b K^2,  K = hat(w),  K^2 = w w^T - theta^2 I
  float R[9];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float ww = fmul(w[j], w[k]);
      R[3 * j + k] = j == k ? fadd(1.0f, fmul(r.b, fsub(ww, th2))) : fmul(r.b, ww);
    }
  const float aw[3] = {fmul(r.a, w[0]), fmul(r.a, w[1]), fmul(r.a, w[2])};
  R[1] = fsub(R[1], aw[2]); R[2] = fadd(R[2], aw[1]);
  R[3] = fadd(R[3], aw[2]); R[5] = fsub(R[5], aw[0]);
  R[6] = fsub(R[6], aw[1]); R[7] = fadd(R[7], aw[0]);
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int k = 0; k < 3; ++k)
      a[3 * j + k] = fadd(fadd(fmul(R[3 * j], base[k]), fmul(R[3 * j + 1], base[4 + k])), fmul(R[3 * j + 2], base[8 + k]));
}

__global__ void pose_exp_kernel(int n_img, const float* __restrict__ base, const float* __restrict__ xi, float* __restrict__ out) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_img; i += gridDim.x * blockDim.x) {
    float b0[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) b0[k] = base[(int64_t)i * 12 + k];
    float x[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (xi) {
#pragma unroll
      for (int k = 0; k < 6; ++k) x[k] = xi[(int64_t)i * 6 + k];
    }
    const float th2 = fadd(fadd(fmul(x[0], x[0]), fmul(x[1], x[1])), fmul(x[2], x[2]));
    float a[9];
    compose(x, th2, rodrigues(th2, false), b0, a);
    float* o = out + (int64_t)i * 12;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
#pragma unroll
      for (int k = 0; k < 3; ++k) o[4 * j + k] = a[3 * j + k];
      o[4 * j + 3] = x[3 + j] == 0.0f ? b0[4 * j + 3] : fadd(b0[4 * j + 3], x[3 + j]);      // (t0 + 0 keeps t0's bits, a -0 too)
    }
  }
}

__global__ void pose_exp_bwd_kernel(int n_img, const float* __restrict__ base, const float* __restrict__ xi,
                                    const float* __restrict__ d_poses, float* __restrict__ d_xi) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_img; i += gridDim.x * blockDim.x) {
    float b0[12], g[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      b0[k] = base[(int64_t)i * 12 + k];
      g[k] = d_poses[(int64_t)i * 12 + k];
    }
    float w[3] = {0.f, 0.f, 0.f};
    if (xi) {
#pragma unroll
      for (int k = 0; k < 3; ++k) w[k] = xi[(int64_t)i * 6 + k];
    }
    const float th2 = fadd(fadd(fmul(w[0], w[0]), fmul(w[1], w[1])), fmul(w[2], w[2]));
    const Rodrigues r = rodrigues(th2, true);
    float a[9];
    compose(w, th2, r, b0, a);
    // s = sum_k A_k x G_k over the columns: a turn phi of the camera moves A by hat(phi) A, so d(loss) = phi . s
    float s[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float ax = a[k], ay = a[3 + k], az = a[6 + k], gx = g[k], gy = g[4 + k], gz = g[8 + k];
      s[0] = fadd(s[0], fsub(fmul(ay, gz), fmul(az, gy)));
      s[1] = fadd(s[1], fsub(fmul(az, gx), fmul(ax, gz)));
      s[2] = fadd(s[2], fsub(fmul(ax, gy), fmul(ay, gx)));
    }
    // d_omega = J_l^T s,  J_l = I + b K + c K^2:  s - b (w x s) + c (w (w . s) - theta^2 s)
    const float ws_ = fadd(fadd(fmul(w[0], s[0]), fmul(w[1], s[1])), fmul(w[2], s[2]));
    const float wxs[3] = {fsub(fmul(w[1], s[2]), fmul(w[2], s[1])), fsub(fmul(w[2], s[0]), fmul(w[0], s[2])),
                          fsub(fmul(w[0], s[1]), fmul(w[1], s[0]))};
    float* o = d_xi + (int64_t)i * 6;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float kk = fsub(fmul(w[j], ws_), fmul(th2, s[j]));
      o[j] = fadd(fsub(s[j], fmul(r.b, wxs[j])), fmul(r.c, kk));
      o[3 + j] = g[4 * j + 3];
    }
  }
}

// ---- pose_grad: d_poses[img] = sum over the rays of image img -----------------------------------------------------------------------
// Workgroup (img, c) walks chunk c of the batch -- a contiguous range of rays, C chunks, C a function of (n, n_img) alone -- and adds the
// rays whose pix row names img: lane t takes rays t, t + 256, ... of the chunk in order, the 256 lane sums meet in a fixed tree (a
// wave's 64 by shuffles, the 4 waves in lane 0), and with C > 1 a second launch adds an image's C partial sums in chunk order.  Which
// lane and which chunk a ray falls to depends on its row index alone: no atomics, bit-identical from call to call.  The walk reads the 4-byte
// image index of every ray of the chunk (out of L2: n_img * n reads in all) and 44 + 8 more bytes of the rays that match.
__global__ void __launch_bounds__(FN_SEG_BLOCK)
pose_grad_kernel(int64_t n, int64_t chunk, const int32_t* __restrict__ pix, const float* __restrict__ poses, float fx, float fy, float cx,
                 float cy, const float* __restrict__ d_rays, float* __restrict__ out) {
  const int img = blockIdx.x, c = blockIdx.y, C = gridDim.y;
  const int64_t lo = c * chunk, hi = (lo + chunk < n) ? lo + chunk : n;
  float pose[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) pose[k] = poses[(int64_t)img * 12 + k];
  float acc[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) acc[k] = 0.0f;
  for (int64_t i = lo + threadIdx.x; i < hi; i += FN_SEG_BLOCK) {
    if (pix[i * 3] != img) continue;
    float dir[3], d[3];
    pixel_dir((float)pix[i * 3 + 1], (float)pix[i * 3 + 2], fx, fy, cx, cy, dir);
    rotate_dir(dir, pose, d);
    const float* g = d_rays + i * 11;
    const float dv[3] = {g[8], g[9], g[10]};
    // g_d = d_d + (d_v - v (v . d_v)) / |d|: the view direction v = d / |d| of pack_rays_kernel, differentiated (d = 0: no such term)
    const float nrm = sqrtf(fadd(fadd(fmul(d[0], d[0]), fmul(d[1], d[1])), fmul(d[2], d[2])));
    float gd[3] = {g[3], g[4], g[5]};
    if (nrm > 0.0f) {
      const float v[3] = {d[0] / nrm, d[1] / nrm, d[2] / nrm};
      const float vd = fadd(fadd(fmul(v[0], dv[0]), fmul(v[1], dv[1])), fmul(v[2], dv[2]));
#pragma unroll
      for (int j = 0; j < 3; ++j) gd[j] = fadd(gd[j], fsub(dv[j], fmul(v[j], vd)) / nrm);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
#pragma unroll
      for (int k = 0; k < 3; ++k) acc[4 * j + k] = fadd(acc[4 * j + k], fmul(gd[j], dir[k]));
      acc[4 * j + 3] = fadd(acc[4 * j + 3], g[j]);
    }
  }
  // 256 -> 1 in the fixed tree of seg_reduce.h
  __shared__ float part[FN_SEG_BLOCK / 64][12];
  seg_wave_sums(acc, part);
  if (threadIdx.x < 12) out[((int64_t)img * C + c) * 12 + threadIdx.x] = seg_total(part, threadIdx.x);
}

// d_poses[img, e] = the sum of the image's C partial sums in chunk order (C == 0: an empty batch, +0)
__global__ void pose_grad_finish_kernel(int n_img, int C, const float* __restrict__ partial, float* __restrict__ d_poses) {
  const int64_t total = (int64_t)n_img * 12;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t img = i / 12;
    const int e = (int)(i % 12);
    float x = 0.0f;
    for (int c = 0; c < C; ++c) x = fadd(x, partial[(img * C + c) * 12 + e]);
    d_poses[i] = x;
  }
}

static inline int lanes_grid(int64_t n, int block = 256) {
  int64_t g = (n + block - 1) / block;
  return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

extern "C" int fastnerf_pose_exp(int n_img, const float* base, const float* xi, float* poses_out, fn_stream_t stream) {
  FN_CHECK_ARG(n_img >= 1, "n_img >= 1");
  FN_CHECK_ARG(base && poses_out, "null pointer (base, poses_out)");
  hipLaunchKernelGGL(pose_exp_kernel, dim3(lanes_grid(n_img, 64)), dim3(64), 0, fn::S(stream), n_img, base, xi, poses_out);
  FN_LAUNCH_CHECK();
  return 0;
}

extern "C" int fastnerf_pose_exp_bwd(int n_img, const float* base, const float* xi, const float* d_poses, float* d_xi,
                                     fn_stream_t stream) {
  FN_CHECK_ARG(n_img >= 1, "n_img >= 1");
  FN_CHECK_ARG(base && d_poses && d_xi, "null pointer (base, d_poses, d_xi)");
  hipLaunchKernelGGL(pose_exp_bwd_kernel, dim3(lanes_grid(n_img, 64)), dim3(64), 0, fn::S(stream), n_img, base, xi, d_poses, d_xi);
  FN_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t fastnerf_pose_grad_ws_floats(int64_t n, int n_img) {
  if (n < 0 || n_img < 1) {
    fn::set_error("fastnerf_pose_grad_ws_floats: bad argument: n >= 0, n_img >= 1");
    return -1;
  }
  const int C = n == 0 ? 0 : seg_chunks(n, n_img);
  return C > 1 ? (int64_t)n_img * C * 12 : 0;
}

extern "C" int fastnerf_pose_grad(int64_t n, int n_img, const int32_t* pix, const float* poses, float fx, float fy, float cx, float cy,
                                  const float* d_rays, float* ws, float* d_poses, fn_stream_t stream) {
  FN_CHECK_ARG(n >= 0, "n >= 0");
  FN_CHECK_ARG(n_img >= 1, "n_img >= 1");
  if (n == 0) {
    if (d_poses) {
      hipLaunchKernelGGL(pose_grad_finish_kernel, dim3(lanes_grid((int64_t)n_img * 12)), dim3(256), 0, fn::S(stream), n_img, 0,
                         (const float*)nullptr, d_poses);
      FN_LAUNCH_CHECK();
    }
    return 0;
  }
  const int C = seg_chunks(n, n_img);
  FN_CHECK_ARG(pix && poses && d_rays && d_poses, "null pointer (pix, poses, d_rays, d_poses)");
  FN_CHECK_ARG(C == 1 || ws, "null pointer (ws: fastnerf_pose_grad_ws_floats(n, n_img) floats)");
  const int64_t chunk = (n + C - 1) / C;
  hipLaunchKernelGGL(pose_grad_kernel, dim3(n_img, C), dim3(FN_SEG_BLOCK), 0, fn::S(stream), n, chunk, pix, poses, fx, fy, cx, cy,
                     d_rays, C == 1 ? d_poses : ws);
  FN_LAUNCH_CHECK();
  if (C > 1) {
    hipLaunchKernelGGL(pose_grad_finish_kernel, dim3(lanes_grid((int64_t)n_img * 12)), dim3(256), 0, fn::S(stream), n_img, C, ws, d_poses);
    FN_LAUNCH_CHECK();
  }
  return 0;
}
