// sigma_grad.hip -- d(sigma)/d(x): the gradient of the density logit with respect to the sample position, for surface normals
// n = -grad / |grad| (mesh.py vertex_normals).
//
// Contract of fastnerf_mlp_sigma_grad (include/fastnerf.h): points o + d*z as in fastnerf_mlp_fwd; the call enqueues
//   1. the SAVING forward of the math mode (raw [P,4], the encoded input `pe` and the ReLU sign words in `act`),
//   2. a fill of the upstream gradient draw[p] = (0, 0, 0, 1): the cotangent of raw[..., 3] alone,
//   3. the dX chain alone (fn_launch_dx_alone / fn_launch_dx_bf16: no dW job, no reduction), which leaves every trunk layer's
//      pre-activation gradient in `dact`,
//   4. sigma_grad_kernel below,
// and writes sigma[p] = raw[p][3] (the logit BEFORE the ReLU of raw2outputs, and so is the gradient) and grad[p][0..2].
//
// What it differentiates (model.py:38-63, run_nerf_helpers.py Embedder):  sigma = alpha_linear(h7),  h0 = relu(W0 pe + b0),
// h5 = relu(W5 [pe, h4] + b5),  pe = [x, sin(2^0 x), cos(2^0 x), ..., sin(2^9 x), cos(2^9 x)] (3 columns each).  The position enters
// through the encoding only, at layer 0 and at the skip layer:
//   dpe[c] = sum_j dY0[j] W0[j][c] + sum_j dY5[j] W5[j][c]                c = 0..62   (W0 256 x 63; W5 256 x 319, the encoding first)
//   g[a]   = dpe[a] + sum_k 2^k (dpe[sin_k,a] pe[cos_k,a] - dpe[cos_k,a] pe[sin_k,a])      sin_k,a = 3 + 6k + a, cos_k,a = 6 + 6k + a
// with the SAVED sines and cosines: no trigonometry is recomputed.
//
// sigma_grad_kernel: one workgroup of four waves per tile of 64 points, any grid order (a point's result depends on its own row only).
//   * dpe [64 x 64] = [dY0 | dY5] [64 x 512] . [W0 ; W5[:, :63]] [512 x 64] on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32
//     accumulation): wave (wm, wn) owns rows 32 wm.., columns 32 wn.. -- one accumulator tile, 256 dependent MFMAs.  The gradients are
//     staged through LDS 64 channels at a time (16 KiB, whole rows read from HBM with 16-byte accesses, the swizzle of mlp_common.h's
//     E layout); the weights (129 KB for both layers, L2 resident) are read straight from the flat parameters, 32 consecutive
//     columns of one row per half wave; column 63 is a zero.
//   * Summation order, fixed: dY0 before dY5, channels ascending in steps of 8; step t = 0..3 of a group adds the products of
//     channels 8i + t and 8i + 4 + t (the two k of one MFMA) to the running sum.  Then, per point and axis, g starts at dpe[a] and
//     takes the ten frequency terms in ASCENDING k; every product and sum is rounded on its own (no contraction).  No atomics:
//     two calls agree bit for bit, wherever the point sits in the batch.
//   * KF = false: the fp32 tensors of the exact-fp32 and bf16x6 modes (dact_y(P, l) + p * 256 + j as mlp_bwd_dw.hip reads them,
//     pe at act_pe + p * 64).  KF = true: the split-bf16 mode's K-fragment tensors (mlp_bf16.hip header): a value is hi + lo of a bf16
//     pair, 8 points per 16 bytes, 256-channel tensors in the wave-permuted channel order.  The mode's arithmetic is in the forward
//     and the dX chain; this kernel only reads what they left.
//   * Cost per point: 2 KiB of dact read (dY0 and dY5, 1 KiB each in both layouts) + 256 B of pe + 16 B written, against
//     2 x 256 x 64 MACs.  At the chip's rates that is 0.37 ns of HBM time (6.3 TB/s achievable) beside 0.42 ns of fp32-MFMA time
//     (155 TFLOP/s): the two floors are within 15 % of each other, neither hides the other entirely, and the 2 KiB of dact is the
//     part no tiling removes.  Several workgroups share a CU (33 KiB of LDS each), so one's loads run under another's MFMAs.
//     Measured shares: profiles/sigma_grad.md.
//   * Rows of a partial last tile are zero-filled on the way into LDS, never read past P where the tensor ends there, never written.
#include "common.h"
#include "mlp_layout.h"

using namespace fnl;
typedef float f32x16 __attribute__((ext_vector_type(16)));

int fn_launch_dx_alone(int mm, int kind, int64_t P, const float* draw, const float* act, const float* params, const float* packed_bwd,
                       float* dact, hipStream_t st);                                                           // mlp_bwd_dx.hip
int fn_launch_dx_bf16(int kind, int64_t P, const float* draw, const float* act_f, const float* params, const float* packed_bwd,
                      float* dact_f, const int* live_idx, const int* live_cnt, hipStream_t st);                // mlp_bf16.hip
void fn_bf16_sigma_grad_offsets(int64_t P, int64_t* pe, int64_t* dy0, int64_t* dy5);                           // mlp_bf16.hip

#define SG_TM 64     // points per tile
#define SG_KC 64     // channels of dY per LDS stage
#define SG_LDP 65    // row stride of the dpe tile (odd: the chain rule reads one row per thread)

// value (point pm of the tile, channel c) of a K-fragment tensor whose tile starts at `t`: hi + lo of the bf16 pair
__device__ __forceinline__ float kf_value(const uint4* __restrict__ t, int pm, int c) {
  const unsigned short* h =
      reinterpret_cast<const unsigned short*>(t + ((((c >> 5) * 4 + (pm >> 4)) * 2) * 64 + ((pm >> 3) & 1) * 32 + (c & 31))) + (pm & 7);
  return __uint_as_float((unsigned)h[0] << 16) + __uint_as_float((unsigned)h[512] << 16);   // lo plane: 64 units = 512 halves on
}

template <bool KF>
__global__ void __launch_bounds__(256)
sigma_grad_kernel(int64_t P, const void* __restrict__ dy0, const void* __restrict__ dy5, const void* __restrict__ pe,
                  const float* __restrict__ raw, const float* __restrict__ W0, const float* __restrict__ W5,
                  float* __restrict__ sigma, float* __restrict__ grad) {
  __shared__ __attribute__((aligned(16))) float Ds[SG_TM * SG_KC];
  __shared__ float Ps[SG_TM * SG_LDP];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int64_t tile = blockIdx.x;
  const int64_t p0 = tile * SG_TM;
  const int valid = (int)((P - p0) < SG_TM ? (P - p0) : SG_TM);
  const int col = wn * 32 + (lane & 31);   // the encoding column of this lane's weights and of its 16 results
  const bool colok = col < 63;
  const int lhalf = lane >> 5;
  const int arow = wm * 32 + (lane & 31);  // the row whose gradients this lane feeds the MFMAs

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

#pragma unroll 1
  for (int seg = 0; seg < 8; ++seg) {      // dY0 channels 0..255, then dY5 channels 0..255, 64 at a time
    const int c0 = (seg & 3) * SG_KC;
    const float* __restrict__ W = seg < 4 ? W0 : W5;
    const int ldw = seg < 4 ? 63 : 319;
    if constexpr (!KF) {
      const float* src = reinterpret_cast<const float*>(seg < 4 ? dy0 : dy5) + p0 * 256 + c0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int e = i * 256 + tid;
        const int m = e >> 4, sl = e & 15;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (m < valid) v = *reinterpret_cast<const float4*>(src + m * 256 + sl * 4);
        *reinterpret_cast<float4*>(Ds + m * SG_KC + ((sl ^ (m & 15)) << 2)) = v;
      }
    } else {
      // channel tiles 2j, 2j + 1 of the permuted order hold the channels 64j .. 64j + 63: channel 64j + 2c + ctl sits at (ctl, c)
      const uint4* src = reinterpret_cast<const uint4*>(seg < 4 ? dy0 : dy5) + tile * 4096 + (c0 >> 5) * 512;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int v = i * 256 + tid;
        const int ctl = v >> 8, ks = (v >> 6) & 3, kb = (v >> 5) & 1, c = v & 31;
        const uint4* q = src + ((ctl * 4 + ks) * 2) * 64 + kb * 32 + c;
        const uint4 h = q[0], l = q[64];
        const unsigned hw[4] = {h.x, h.y, h.z, h.w}, lw[4] = {l.x, l.y, l.z, l.w};
        const int ln = 2 * c + ctl, m0 = ks * 16 + kb * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const unsigned hb = (e & 1) ? (hw[e >> 1] & 0xffff0000u) : (hw[e >> 1] << 16);
          const unsigned lb = (e & 1) ? (lw[e >> 1] & 0xffff0000u) : (lw[e >> 1] << 16);
          const int m = m0 + e;
          const float val = __uint_as_float(hb) + __uint_as_float(lb);
          Ds[m * SG_KC + ((((ln >> 2) ^ (m & 15)) << 2) | (ln & 3))] = m < valid ? val : 0.f;
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < SG_KC / 8; ++ks) {
      const float4 a = *reinterpret_cast<const float4*>(Ds + arow * SG_KC + (((ks * 2 + lhalf) ^ (arow & 15)) << 2));
      const float* wrow = W + (int64_t)(c0 + ks * 8 + lhalf * 4) * ldw + col;
      float b[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) b[t] = colok ? wrow[t * ldw] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b[0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b[1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b[2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b[3], acc, 0, 0, 0);
    }
    __syncthreads();
  }
  // C layout of v_mfma_f32_32x32x2_f32: column lane & 31, row (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int r = 0; r < 16; ++r) Ps[(wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhalf) * SG_LDP + col] = acc[r];
  __syncthreads();
  // chain rule through the encoding: thread (point pm, axis a); a == 3 copies the logit
  const int pm = tid >> 2, a = tid & 3;
  if (pm >= valid) return;
  const int64_t p = p0 + pm;
  if (a == 3) {
    if (sigma != nullptr) sigma[p] = raw[p * 4 + 3];
    return;
  }
  const float* d = Ps + pm * SG_LDP;
  float g = d[a];
#pragma unroll
  for (int k = 0; k < 10; ++k) {
    const int cs = 3 + 6 * k + a, cc = 6 + 6 * k + a;
    float ps, pc;
    if constexpr (KF) {
      const uint4* t = reinterpret_cast<const uint4*>(pe) + tile * 1024;
      ps = kf_value(t, pm, cs);
      pc = kf_value(t, pm, cc);
    } else {
      const float* e = reinterpret_cast<const float*>(pe) + p * 64;
      ps = e[cs];
      pc = e[cc];
    }
    g = fadd(g, fmul((float)(1 << k), fsub(fmul(d[cs], pc), fmul(d[cc], ps))));
  }
  grad[p * 3 + a] = g;
}

// draw[p] = (0, 0, 0, 1): the cotangent that selects the density logit
__global__ void __launch_bounds__(256) sigma_cotangent_kernel(int64_t P, float4* __restrict__ draw) {
  const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (p < P) draw[p] = make_float4(0.f, 0.f, 0.f, 1.f);
}

static inline int64_t up4(int64_t v) { return (v + 3) / 4 * 4; }
static int64_t sg_act_floats(int math_mode, int64_t P) {
  return up4(math_mode == 1 ? fastnerf_mlp_bf16_floats(0, 3, P) : fastnerf_mlp_act_floats(0, P));
}
static int64_t sg_dact_floats(int math_mode, int64_t P) {
  return up4(math_mode == 1 ? fastnerf_mlp_bf16_floats(0, 4, P) : P * (int64_t)FASTNERF_DACT_FLOATS);
}

// sigma_grad_kernel on a caller's saved activations and pre-activation gradients of P points (the layouts of `math_mode`): what
// fastnerf_mlp_sigma_grad runs on its own scratch, and fastnerf_ray_grad (ray_grad.hip) on the scratch a training backward left, whose
// dY0 / dY5 then hold the cotangent of a loss instead of (0, 0, 0, 1).  raw is read only when sigma is wanted.
int fn_launch_sigma_grad(int math_mode, int64_t P, const float* act, const float* dact, const float* raw, const float* params,
                         float* sigma, float* grad, hipStream_t st) {
  const NetLayout L = make_layout(0);
  const unsigned grid = (unsigned)((P + SG_TM - 1) / SG_TM);
  if (math_mode == 1) {
    int64_t ope, oy0, oy5;
    fn_bf16_sigma_grad_offsets(P, &ope, &oy0, &oy5);
    const uint4* a4 = reinterpret_cast<const uint4*>(act);
    const uint4* d4 = reinterpret_cast<const uint4*>(dact);
    hipLaunchKernelGGL(sigma_grad_kernel<true>, dim3(grid), dim3(256), 0, st, P, static_cast<const void*>(d4 + oy0),
                       static_cast<const void*>(d4 + oy5), static_cast<const void*>(a4 + ope), static_cast<const float*>(raw),
                       params + L.LW[0], params + L.LW[5], sigma, grad);
  } else {
    hipLaunchKernelGGL(sigma_grad_kernel<false>, dim3(grid), dim3(256), 0, st, P, static_cast<const void*>(dact + dact_y(P, 0)),
                       static_cast<const void*>(dact + dact_y(P, 5)), static_cast<const void*>(act + act_pe(P, L.pe_pad)),
                       static_cast<const float*>(raw), params + L.LW[0], params + L.LW[5], sigma, grad);
  }
  FN_LAUNCH_CHECK();
  return 0;
}

// act | dact | draw [P,4] | raw [P,4], each part 16-byte aligned
extern "C" int64_t fastnerf_mlp_sigma_grad_ws_floats(int math_mode, int64_t n_points) {
  if (math_mode < 0 || math_mode > 2 || n_points < 0) {
    fn::set_error("fastnerf_mlp_sigma_grad_ws_floats: bad argument: math_mode in {0,1,2}, n_points>=0");
    return -1;
  }
  return sg_act_floats(math_mode, n_points) + sg_dact_floats(math_mode, n_points) + 8 * n_points;
}

extern "C" int fastnerf_mlp_sigma_grad(int math_mode, int kind, int64_t n, int S, const float* rays11, const float* z,
                                       const float* params, const float* packed_fwd, const float* packed_bwd, float* ws,
                                       float* sigma, float* grad, fn_stream_t stream) {
  FN_CHECK_ARG(math_mode >= 0 && math_mode <= 2 && n > 0 && S >= 1, "math_mode in {0,1,2}, n>0, S>=1");
  if (kind != 0) {
    fn::set_error("fastnerf_mlp_sigma_grad: kind %d is not supported: the density gradient exists for kind 0 (NeRF) only", kind);
    return -1;
  }
  FN_CHECK_ARG(rays11 && z && params && packed_fwd && packed_bwd && ws && grad, "null pointer");
  const int64_t P = n * S;
  float* act = ws;
  float* dact = act + sg_act_floats(math_mode, P);
  float* draw = dact + sg_dact_floats(math_mode, P);
  float* raw = draw + 4 * P;
  hipStream_t st = fn::S(stream);
  int rc;
  if (math_mode == 0) rc = fastnerf_mlp_fwd_ex(0, n, S, rays11, z, params, packed_fwd, raw, act, stream);
  else if (math_mode == 1) rc = fastnerf_mlp_bf16_fwd(0, n, S, rays11, z, params, packed_fwd, raw, act, stream);
  else rc = fastnerf_mlp_x6_fwd(0, n, S, rays11, z, params, packed_fwd, raw, act, 0, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(sigma_cotangent_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, P, reinterpret_cast<float4*>(draw));
  FN_LAUNCH_CHECK();
  if (math_mode == 1) rc = fn_launch_dx_bf16(0, P, draw, act, params, packed_bwd, dact, nullptr, nullptr, st);
  else rc = fn_launch_dx_alone(math_mode == 2 ? 1 : 0, 0, P, draw, act, params, packed_bwd, dact, st);
  if (rc) return rc;
  return fn_launch_sigma_grad(math_mode, P, act, dact, raw, params, sigma, grad, st);
}
