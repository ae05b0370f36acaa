// envmap.hip -- a learned environment map: a table of colours indexed by ray direction alone, put behind the volume as the injected
// per-ray background (include/fastnerf.h, "environment map"), for gfx950.  The table T [R,R,3] is an octahedral map; for ray r:
//   fastnerf_env_lookup   out[r] = the bilinear sample of T at the octahedral image of d_r, mirror-wrapped at the table's border;
//   fastnerf_env_grad     what rgb_p += (1 - acc_p) env(d) sends back to T: per ray and channel g = (1-acc1) g_rgb1 + (1-acc0) g_rgb0,
//                         its four terms w_k g scattered to their texels.
// tests/env_ref.py restates both operation for operation.
//
// Only + - * / and comparisons, every one rounded on its own (fmul / fadd / fsub of common.h, one IEEE division): no atan2 or acos whose
// last bits would decide a texel.  The lookup is one thread per ray in a grid-stride walk, plain vector stores.  The scatter's destination
// depends on the data, so the segmented sums of seg_reduce.h do not apply; every term is rounded ONCE to a multiple of 2^-50 and added as
// a 64-bit integer with a vector atomic to global memory (the device of leaf_sumcount_kernel, in integer form).  Integer addition is
// associative: the result is the same bits whatever the arrival order, the order of the rays or the split of a batch.
// Bounds: a lane touches words dirs[r*stride + 0..2], rows r < n of the [n,3] and [n] buffers, and texels (j,i) with both indices clamped
// to [0, R) before any address is formed.
#include "common.h"

#define ENV_BLOCK 256
#define ENV_MAX_GRID 256          // 65 536 lanes in flight; longer batches are walked in strides of the grid
#define ENV_MAX_R 16384           // R*R*3 words stay below 2^31
#define ENV_FIX 1125899906842624.0      // 2^50

namespace {

struct EnvTap {
  int64_t t[4];      // word offsets of the four texels' channel 0: (i0,j0), (i0+1,j0), (i0,j0+1), (i0+1,j0+1)
  float w[4];
};

__device__ __forceinline__ float env_sg(float t) { return t >= 0.0f ? 1.0f : -1.0f; }      // -0 -> +1

// texel (i, j), either index possibly one outside [0, R): the octahedral map's identification of its border
__device__ __forceinline__ int64_t env_texel(int i, int j, int R) {
  const bool oi = i < 0 || i >= R, oj = j < 0 || j >= R;
  i = i < 0 ? 0 : (i >= R ? R - 1 : i);
  j = j < 0 ? 0 : (j >= R ? R - 1 : j);
  if (oi) j = R - 1 - j;
  if (oj) i = R - 1 - i;
  return ((int64_t)j * R + i) * 3;
}

__device__ __forceinline__ void env_cell(float p, float Rf, int R, int* i0, float* f) {
  const float x = fsub(fmul(fadd(fmul(p, 0.5f), 0.5f), Rf), 0.5f);
  float fl = floorf(x);
  fl = !(fl >= -1.0f) ? -1.0f : (fl > Rf ? Rf : fl);      // |p| <= 1 puts x in [-0.5, R-0.5]: the clamp never acts, it keeps (int) defined
  *i0 = (int)fl;
  *f = fsub(x, fl);
}

__device__ __forceinline__ void env_taps(const float* __restrict__ d, int R, EnvTap* tap) {
  const float dx = d[0], dy = d[1], dz = d[2];
  const float s = fadd(fadd(fabsf(dx), fabsf(dy)), fabsf(dz));
  float px = 0.0f, py = 0.0f;
  if (s != 0.0f && s - s == 0.0f) {      // not zero, and finite
    px = __fdiv_rn(dx, s);
    py = __fdiv_rn(dy, s);
  }
  if (dz < 0.0f) {      // (also behind p = (0, 0): the -z pole, a corner)
    const float qx = fmul(fsub(1.0f, fabsf(py)), env_sg(px));
    const float qy = fmul(fsub(1.0f, fabsf(px)), env_sg(py));
    px = qx;
    py = qy;
  }
  const float Rf = (float)R;
  int i0, j0;
  float fx, fy;
  env_cell(px, Rf, R, &i0, &fx);
  env_cell(py, Rf, R, &j0, &fy);
  tap->t[0] = env_texel(i0, j0, R);
  tap->t[1] = env_texel(i0 + 1, j0, R);
  tap->t[2] = env_texel(i0, j0 + 1, R);
  tap->t[3] = env_texel(i0 + 1, j0 + 1, R);
  const float gx = fsub(1.0f, fx), gy = fsub(1.0f, fy);
  tap->w[0] = fmul(gx, gy);
  tap->w[1] = fmul(fx, gy);
  tap->w[2] = fmul(gx, fy);
  tap->w[3] = fmul(fx, fy);
}

__global__ void __launch_bounds__(ENV_BLOCK) env_lookup_kernel(int64_t n, const float* __restrict__ dirs, int64_t stride,
                                                               const float* __restrict__ table, int R, float* __restrict__ out) {
  for (int64_t r = blockIdx.x * (int64_t)ENV_BLOCK + threadIdx.x; r < n; r += (int64_t)gridDim.x * ENV_BLOCK) {
    EnvTap tap;
    env_taps(dirs + r * stride, R, &tap);
#pragma unroll
    for (int c = 0; c < 3; ++c)
      out[r * 3 + c] = fadd(fadd(fmul(tap.w[0], table[tap.t[0] + c]), fmul(tap.w[1], table[tap.t[1] + c])),
                            fadd(fmul(tap.w[2], table[tap.t[2] + c]), fmul(tap.w[3], table[tap.t[3] + c])));
  }
}

__global__ void __launch_bounds__(ENV_BLOCK) env_zero_kernel(int64_t words, unsigned long long* __restrict__ ws) {
  for (int64_t t = blockIdx.x * (int64_t)ENV_BLOCK + threadIdx.x; t < words; t += (int64_t)gridDim.x * ENV_BLOCK) ws[t] = 0ull;
}

__global__ void __launch_bounds__(ENV_BLOCK) env_scatter_kernel(int64_t n, const float* __restrict__ dirs, int64_t stride, int R,
                                                                const float* __restrict__ g_rgb1, const float* __restrict__ acc1,
                                                                const float* __restrict__ g_rgb0, const float* __restrict__ acc0,
                                                                unsigned long long* __restrict__ ws) {
  for (int64_t r = blockIdx.x * (int64_t)ENV_BLOCK + threadIdx.x; r < n; r += (int64_t)gridDim.x * ENV_BLOCK) {
    EnvTap tap;
    env_taps(dirs + r * stride, R, &tap);
    const float t1 = fsub(1.0f, acc1[r]);
    const float t0 = g_rgb0 ? fsub(1.0f, acc0[r]) : 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float g = fmul(t1, g_rgb1[r * 3 + c]);
      if (g_rgb0) g = fadd(g, fmul(t0, g_rgb0[r * 3 + c]));
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long long q = __double2ll_rn((double)fmul(tap.w[k], g) * ENV_FIX);
        if (q != 0) atomicAdd(ws + tap.t[k] + c, (unsigned long long)q);      // two's complement: the sum is the signed sum
      }
    }
  }
}

__global__ void __launch_bounds__(ENV_BLOCK) env_finish_kernel(int64_t words, const unsigned long long* __restrict__ ws,
                                                               float* __restrict__ d_table) {
  for (int64_t t = blockIdx.x * (int64_t)ENV_BLOCK + threadIdx.x; t < words; t += (int64_t)gridDim.x * ENV_BLOCK)
    d_table[t] = (float)((double)(long long)ws[t] * (1.0 / ENV_FIX));
}

inline int env_grid(int64_t n) {
  int64_t g = (n + ENV_BLOCK - 1) / ENV_BLOCK;
  return (int)(g < 1 ? 1 : (g > ENV_MAX_GRID ? ENV_MAX_GRID : g));
}

}  // namespace

extern "C" int fastnerf_env_lookup(int64_t n, const float* dirs, int64_t stride, const float* table, int R, float* out,
                                   fn_stream_t stream) {
  FN_CHECK_ARG(n >= 0, "n >= 0");
  FN_CHECK_ARG(R >= 2 && R <= ENV_MAX_R, "2 <= R <= 16384");
  FN_CHECK_ARG(stride >= 3, "stride >= 3");
  if (n == 0) return 0;
  FN_CHECK_ARG(dirs && table && out, "null pointer (dirs, table, out)");
  hipLaunchKernelGGL(env_lookup_kernel, dim3(env_grid(n)), dim3(ENV_BLOCK), 0, fn::S(stream), n, dirs, stride, table, R, out);
  FN_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t fastnerf_env_grad_ws_bytes(int R) {
  if (R < 2 || R > ENV_MAX_R) {
    fn::set_error("fastnerf_env_grad_ws_bytes: bad argument: 2 <= R <= 16384");
    return -1;
  }
  return (int64_t)R * R * 3 * (int64_t)sizeof(int64_t);
}

extern "C" int fastnerf_env_grad(int64_t n, const float* dirs, int64_t stride, int R, const float* g_rgb1, const float* acc1,
                                 const float* g_rgb0, const float* acc0, void* ws, float* d_table, fn_stream_t stream) {
  FN_CHECK_ARG(n >= 0, "n >= 0");
  FN_CHECK_ARG(R >= 2 && R <= ENV_MAX_R, "2 <= R <= 16384");
  FN_CHECK_ARG(stride >= 3, "stride >= 3");
  FN_CHECK_ARG(d_table, "null pointer (d_table)");
  FN_CHECK_ARG(n == 0 || (dirs && g_rgb1 && acc1 && ws), "null pointer (dirs, g_rgb1, acc1, ws)");
  FN_CHECK_ARG((g_rgb0 != nullptr) == (acc0 != nullptr), "g_rgb0 and acc0 go together");
  FN_CHECK_ARG(n == 0 || ((uintptr_t)ws & 7) == 0, "ws: 8-byte aligned");
  const int64_t words = (int64_t)R * R * 3;
  if (n == 0) {
    FN_HIP(hipMemsetAsync(d_table, 0, (size_t)words * sizeof(float), fn::S(stream)));
    return 0;
  }
  unsigned long long* w = static_cast<unsigned long long*>(ws);
  hipLaunchKernelGGL(env_zero_kernel, dim3(env_grid(words)), dim3(ENV_BLOCK), 0, fn::S(stream), words, w);
  FN_LAUNCH_CHECK();
  hipLaunchKernelGGL(env_scatter_kernel, dim3(env_grid(n)), dim3(ENV_BLOCK), 0, fn::S(stream), n, dirs, stride, R, g_rgb1, acc1, g_rgb0,
                     acc0, w);
  FN_LAUNCH_CHECK();
  hipLaunchKernelGGL(env_finish_kernel, dim3(env_grid(words)), dim3(ENV_BLOCK), 0, fn::S(stream), words, w, d_table);
  FN_LAUNCH_CHECK();
  return 0;
}
