// bkgd.hip -- per-ray background colours (include/fastnerf.h, "per-ray background colours"), for gfx950.  The compositing kernels know one
// background, white; any other colour b_r is put behind a ray AFTER a compositing with white_bkgd = 0:
//   fastnerf_bkgd_blend   rgb_r += (1 - acc_r) b_r on the maps of one or two passes, the target blended over the same colour through its
//                         alpha, and the colours that were used written out (drawn here when the caller injects none);
//   fastnerf_bkgd_grad    what the blend sends back to acc_r: g_acc_r = add_r - (g_rgb_r . b_r), the row that the full-gradient compositing
//                         backward (fastnerf_raw2outputs_bwd_full) takes beside g_rgb.
// tests/bkgd_ref.py restates both operation for operation.
//
// One thread per ray, 256 per block, no LDS, no atomics, plain vector stores: bit-identical from call to call, and a ray's result does
// not depend on where it sits in the batch.  Every product and sum is rounded on its own (fmul / fadd / fsub of common.h): with b = 1
// the colour line has the bits of the white branch of raw2outputs_fwd_kernel, and the target line those of the loader's white composite.
// Bounds: thread r < n touches rows r of [n,3] and [n] buffers only.
#include "common.h"

#define BKGD_BLOCK 256

namespace {

// b_r from the caller's buffer, or u01 of words 0..2 of Philox block r of the stream 'bkgd' ("Random streams")
__device__ __forceinline__ void bkgd_colour(const float* bkgd, uint64_t seed, int64_t r, float b[3]) {
  if (bkgd) {
    b[0] = bkgd[r * 3]; b[1] = bkgd[r * 3 + 1]; b[2] = bkgd[r * 3 + 2];
    return;
  }
  uint32_t o[4];
  philox4x32((uint32_t)r, (uint32_t)((uint64_t)r >> 32), 0x626b6764u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), o);
  b[0] = u01(o[0]); b[1] = u01(o[1]); b[2] = u01(o[2]);
}

__global__ void __launch_bounds__(BKGD_BLOCK) bkgd_blend_kernel(int64_t n, const float* bkgd, uint64_t seed, const float* alpha,
                                                                const float* acc1, const float* acc0, float* rgb1, float* rgb0,
                                                                const float* target, float* target_out, float* bkgd_used) {
  const int64_t r = (int64_t)blockIdx.x * BKGD_BLOCK + threadIdx.x;
  if (r >= n) return;
  float b[3];
  bkgd_colour(bkgd, seed, r, b);
  const float t1 = fsub(1.0f, acc1[r]);
  const float t0 = rgb0 ? fsub(1.0f, acc0[r]) : 0.f;
  const float a = alpha ? alpha[r] : 1.0f;
  const float ta = fsub(1.0f, a);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    rgb1[r * 3 + c] = fadd(rgb1[r * 3 + c], fmul(t1, b[c]));
    if (rgb0) rgb0[r * 3 + c] = fadd(rgb0[r * 3 + c], fmul(t0, b[c]));
    const float t = target[r * 3 + c];
    target_out[r * 3 + c] = alpha ? fadd(fmul(t, a), fmul(ta, b[c])) : t;
    bkgd_used[r * 3 + c] = b[c];
  }
}

__global__ void __launch_bounds__(BKGD_BLOCK) bkgd_grad_kernel(int64_t n, const float* bkgd_used, const float* g_rgb1, const float* g_rgb0,
                                                               const float* add1, const float* add0, float* g_acc1, float* g_acc0) {
  const int64_t r = (int64_t)blockIdx.x * BKGD_BLOCK + threadIdx.x;
  if (r >= n) return;
  const float b0 = bkgd_used[r * 3], b1 = bkgd_used[r * 3 + 1], b2 = bkgd_used[r * 3 + 2];
  const float x1 = fadd(fadd(fmul(g_rgb1[r * 3], b0), fmul(g_rgb1[r * 3 + 1], b1)), fmul(g_rgb1[r * 3 + 2], b2));
  g_acc1[r] = add1 ? fsub(add1[r], x1) : -x1;
  if (g_rgb0) {
    const float x0 = fadd(fadd(fmul(g_rgb0[r * 3], b0), fmul(g_rgb0[r * 3 + 1], b1)), fmul(g_rgb0[r * 3 + 2], b2));
    g_acc0[r] = add0 ? fsub(add0[r], x0) : -x0;
  }
}

}  // namespace

extern "C" int fastnerf_bkgd_blend(int64_t n, const float* bkgd, uint64_t seed, const float* alpha, const float* acc1, const float* acc0,
                                   float* rgb1, float* rgb0, const float* target, float* target_out, float* bkgd_used,
                                   fn_stream_t stream) {
  FN_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31), "0 <= n < 2^31");
  FN_CHECK_ARG((bkgd != nullptr) != (seed != 0), "exactly one of bkgd and seed != 0");
  if (n == 0) return 0;
  FN_CHECK_ARG(acc1 && rgb1 && target && target_out && bkgd_used, "non-null pointers");
  FN_CHECK_ARG((rgb0 != nullptr) == (acc0 != nullptr), "rgb0 and acc0 go together");
  hipLaunchKernelGGL(bkgd_blend_kernel, dim3((unsigned)((n + BKGD_BLOCK - 1) / BKGD_BLOCK)), dim3(BKGD_BLOCK), 0, fn::S(stream), n, bkgd,
                     seed, alpha, acc1, acc0, rgb1, rgb0, target, target_out, bkgd_used);
  FN_LAUNCH_CHECK();
  return 0;
}

extern "C" int fastnerf_bkgd_grad(int64_t n, const float* bkgd_used, const float* g_rgb1, const float* g_rgb0, const float* add1,
                                  const float* add0, float* g_acc1, float* g_acc0, fn_stream_t stream) {
  FN_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31), "0 <= n < 2^31");
  if (n == 0) return 0;
  FN_CHECK_ARG(bkgd_used && g_rgb1 && g_acc1, "non-null pointers");
  FN_CHECK_ARG(!g_rgb0 || g_acc0, "g_acc0 with g_rgb0");
  hipLaunchKernelGGL(bkgd_grad_kernel, dim3((unsigned)((n + BKGD_BLOCK - 1) / BKGD_BLOCK)), dim3(BKGD_BLOCK), 0, fn::S(stream), n,
                     bkgd_used, g_rgb1, g_rgb0, add1, add0, g_acc1, g_acc0);
  FN_LAUNCH_CHECK();
  return 0;
}
