// exposure.hip -- a table of per-image exposures that training fits beside the field (include/fastnerf.h, "exposure table"), for gfx950.
// Row i of ab [n_img,2] is (a_i, shift_i); scale_i = |a_i| + 0.5, so that the row (0.5, 0) is the identity.  For ray r of image i = img[r]:
//   fastnerf_expo_apply   e_p[r,c] = (rgb_p[r,c] - shift_i) / scale_i on the maps of one or two passes -- what the colour loss sees;
//   fastnerf_expo_grad    what that loss sends back: g_p = G_p / scale_i written over G_p IN PLACE (the colour gradient the backward reads),
//                         d_shift_i = -sum g, d_scale_i = -sum g e over the rays of image i, and the L1 pull of the table towards (1, 0).
// tests/expo_ref.py restates both operation for operation.
//
// Every product, sum and difference is rounded on its own (fmul / fadd / fsub of common.h), the division is one IEEE division: with the
// identity row e has the bits of rgb (x - 0) and g those of G (x / 1).  A ray whose img lies outside [0, n_img) is left as it is by both
// kernels (e = rgb, g = G) and belongs to no image: no table row is read for it.  No atomics, plain vector stores: bit-identical from call
// to call.  The per-image sums are the segmented sum of seg_reduce.h; every ray is owned by exactly one workgroup -- (img[r], the chunk r
// lies in) -- so the in-place write of g is race-free.
// Bounds: a lane touches rows r < n of the [n,3] and [n] buffers, row i < n_img of ab, and its own workgroup's 3 words of ws.
#include "common.h"
#include "seg_reduce.h"

#define EXPO_BLOCK 256

namespace {

__device__ __forceinline__ float expo_scale(float a) { return fadd(fabsf(a), 0.5f); }
__device__ __forceinline__ float sign_f(float x) { return (float)((x > 0.0f) - (x < 0.0f)); }      // sign(0) = 0, as torch.abs differentiates

__global__ void __launch_bounds__(EXPO_BLOCK) expo_apply_kernel(int64_t n, int n_img, const int32_t* __restrict__ img,
                                                                const float* __restrict__ ab, const float* __restrict__ rgb1,
                                                                const float* __restrict__ rgb0, float* __restrict__ e1,
                                                                float* __restrict__ e0) {
  const int64_t r = (int64_t)blockIdx.x * EXPO_BLOCK + threadIdx.x;
  if (r >= n) return;
  const int32_t i = img[r];
  const bool in = i >= 0 && i < n_img;
  const float scale = in ? expo_scale(ab[2 * (int64_t)i]) : 1.0f;
  const float shift = in ? ab[2 * (int64_t)i + 1] : 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float x1 = rgb1[r * 3 + c];
    e1[r * 3 + c] = in ? __fdiv_rn(fsub(x1, shift), scale) : x1;
    if (rgb0) {
      const float x0 = rgb0[r * 3 + c];
      e0[r * 3 + c] = in ? __fdiv_rn(fsub(x0, shift), scale) : x0;
    }
  }
}

// workgroup (image, chunk): the rays of its chunk that name its image; partial [n_img, C, 3] = (sum g, sum g e, the number of rays as int32)
__global__ void __launch_bounds__(FN_SEG_BLOCK) expo_grad_kernel(int64_t n, int64_t chunk, const int32_t* __restrict__ img,
                                                                 const float* __restrict__ ab, const float* __restrict__ e1,
                                                                 const float* __restrict__ e0, float* g1, float* g0,
                                                                 float* __restrict__ partial) {
  const int image = blockIdx.x, c = blockIdx.y, C = gridDim.y;
  const int64_t lo = c * chunk, hi = (lo + chunk < n) ? lo + chunk : n;
  const float scale = expo_scale(ab[2 * (int64_t)image]);
  float acc[2] = {0.0f, 0.0f};      // sum g, sum g e: the image pass's three channels, then the coarse pass's
  int32_t cnt[1] = {0};
  for (int64_t r = lo + threadIdx.x; r < hi; r += FN_SEG_BLOCK) {
    if (img[r] != image) continue;
    cnt[0] += 1;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float g = __fdiv_rn(g1[r * 3 + k], scale);
      g1[r * 3 + k] = g;
      acc[0] = fadd(acc[0], g);
      acc[1] = fadd(acc[1], fmul(g, e1[r * 3 + k]));
    }
    if (g0) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float g = __fdiv_rn(g0[r * 3 + k], scale);
        g0[r * 3 + k] = g;
        acc[0] = fadd(acc[0], g);
        acc[1] = fadd(acc[1], fmul(g, e0[r * 3 + k]));
      }
    }
  }
  __shared__ float part[FN_SEG_BLOCK / 64][2];
  __shared__ int32_t part_n[FN_SEG_BLOCK / 64][1];
  seg_wave_sums(acc, part);
  seg_wave_sums(cnt, part_n);
  float* o = partial + ((int64_t)image * C + c) * 3;
  if (threadIdx.x < 2) o[threadIdx.x] = seg_total(part, threadIdx.x);
  if (threadIdx.x == 2) reinterpret_cast<int32_t*>(o)[2] = seg_total(part_n, 0);
}

// One workgroup, the images in tiles of 256.  Per image: the C partial sums in chunk order, the sign and penalty lines, counts, and its term of
// the penalty into LDS; then lane 0 adds the tile's terms in index order (an image without a ray: +0).  C == 0: an empty batch, zeros.
__global__ void __launch_bounds__(EXPO_BLOCK) expo_finish_kernel(int64_t n, int n_img, int C, const float* __restrict__ ab, float lambda,
                                                                 float grad_scale, const float* __restrict__ partial,
                                                                 float* __restrict__ d_ab, int32_t* __restrict__ counts,
                                                                 float* __restrict__ loss_reg) {
  __shared__ float term[EXPO_BLOCK];
  const float nf = (float)n;
  float reg = 0.0f;      // (lane 0's)
  for (int64_t base = 0; base < n_img; base += EXPO_BLOCK) {
    const int64_t i = base + threadIdx.x;
    float t = 0.0f;
    if (i < n_img) {
      float s_g = 0.0f, s_ge = 0.0f;
      int32_t m = 0;
      for (int c = 0; c < C; ++c) {
        const float* p = partial + (i * C + c) * 3;
        s_g = fadd(s_g, p[0]);
        s_ge = fadd(s_ge, p[1]);
        m += reinterpret_cast<const int32_t*>(p)[2];
      }
      counts[i] = m;
      float d_a = 0.0f, d_shift = 0.0f;      // an image without a ray: an exact zero row
      if (m != 0) {
        const float a = ab[2 * i], shift = ab[2 * i + 1];
        const float off = fsub(expo_scale(a), 1.0f);
        const float frac = __fdiv_rn((float)m, nf);
        const float pen = fmul(fmul(lambda, grad_scale), frac);
        d_a = fmul(sign_f(a), fadd(-s_ge, fmul(pen, sign_f(off))));
        d_shift = fadd(-s_g, fmul(pen, sign_f(shift)));
        t = fmul(frac, fadd(fabsf(off), fabsf(shift)));
      }
      d_ab[2 * i] = d_a;
      d_ab[2 * i + 1] = d_shift;
    }
    term[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int k1 = (n_img - base < EXPO_BLOCK) ? (int)(n_img - base) : EXPO_BLOCK;
      for (int k = 0; k < k1; ++k) reg = fadd(reg, term[k]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) loss_reg[0] = reg;
}

}  // namespace

extern "C" int fastnerf_expo_apply(int64_t n, int n_img, const int32_t* img, const float* ab, const float* rgb1, const float* rgb0,
                                   float* e1, float* e0, fn_stream_t stream) {
  FN_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31), "0 <= n < 2^31");
  FN_CHECK_ARG(n_img >= 1, "n_img >= 1");
  if (n == 0) return 0;
  FN_CHECK_ARG(img && ab && rgb1 && e1, "null pointer (img, ab, rgb1, e1)");
  FN_CHECK_ARG((rgb0 != nullptr) == (e0 != nullptr), "rgb0 and e0 go together");
  hipLaunchKernelGGL(expo_apply_kernel, dim3((unsigned)((n + EXPO_BLOCK - 1) / EXPO_BLOCK)), dim3(EXPO_BLOCK), 0, fn::S(stream), n, n_img,
                     img, ab, rgb1, rgb0, e1, e0);
  FN_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t fastnerf_expo_grad_ws_floats(int64_t n, int n_img) {
  if (n < 0 || n >= ((int64_t)1 << 31) || n_img < 1) {
    fn::set_error("fastnerf_expo_grad_ws_floats: bad argument: 0 <= n < 2^31, n_img >= 1");
    return -1;
  }
  return n == 0 ? 0 : (int64_t)n_img * seg_chunks(n, n_img) * 3;
}

extern "C" int fastnerf_expo_grad(int64_t n, int n_img, const int32_t* img, const float* ab, float lambda, float grad_scale,
                                  const float* e1, const float* e0, float* g1, float* g0, float* ws, float* d_ab, int32_t* counts,
                                  float* loss_reg, fn_stream_t stream) {
  FN_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31), "0 <= n < 2^31");
  FN_CHECK_ARG(n_img >= 1, "n_img >= 1");
  FN_CHECK_ARG(lambda >= 0.0f && lambda < __builtin_huge_valf(), "lambda >= 0 and finite");
  FN_CHECK_ARG(ab && d_ab && counts && loss_reg, "null pointer (ab, d_ab, counts, loss_reg)");
  FN_CHECK_ARG(n == 0 || (img && e1 && g1), "null pointer (img, e1, g1)");
  FN_CHECK_ARG(n == 0 || (e0 != nullptr) == (g0 != nullptr), "e0 and g0 go together");
  FN_CHECK_ARG(n == 0 || ws, "null pointer (ws: fastnerf_expo_grad_ws_floats(n, n_img) floats)");
  const int C = n == 0 ? 0 : seg_chunks(n, n_img);
  if (C > 0) {
    const int64_t chunk = (n + C - 1) / C;
    hipLaunchKernelGGL(expo_grad_kernel, dim3(n_img, C), dim3(FN_SEG_BLOCK), 0, fn::S(stream), n, chunk, img, ab, e1, e0, g1, g0, ws);
    FN_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(expo_finish_kernel, dim3(1), dim3(EXPO_BLOCK), 0, fn::S(stream), n, n_img, C, ab, lambda, grad_scale, ws, d_ab, counts,
                     loss_reg);
  FN_LAUNCH_CHECK();
  return 0;
}
