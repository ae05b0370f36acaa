// bands.hip -- per-band weights of the positional encoding (include/fastnerf.h, "band weights"), for gfx950.  A weighted encoding
// w (.) gamma(x) enters a network through three matrices only -- layer 0, the skip layer and the view layer -- and W (w (.) gamma) =
// (W diag(w)) gamma, so the MLP kernels run unchanged on an EFFECTIVE network whose encoding columns are the master's times w:
//   fastnerf_band_apply   effective = master, bit for bit, except LW[0][:, 0:in_pe], LW[5][:, 0:in_pe] (times w_pos[col]) and
//                         VW[:, 256:283] (times w_view[col - 256]): one fp32 multiply there, no multiply anywhere else;
//   fastnerf_band_grad    the same three regions of a gradient buffer times the same weights, in place: the chain rule of the line above.
// tests/bands_ref.py restates both.
//
// band_apply is one grid-stride walk over the n_params floats of the net: consecutive lanes read and write consecutive floats, whatever the
// rows' lengths (63, 319 and 283 floats: no row is 16-byte aligned, so the accesses stay scalar).  The weights (at most 84 + 27 floats) stay in
// cache.  band_grad walks the 2 * 256 * in_pe + 128 * 27 floats of the regions alone.  No LDS, no atomics, plain vector stores.
// Bounds: element e < n_params of master / effective; column c < in_pe of w_pos, c - 256 < 27 of w_view; offsets from layout_of(kind) alone.
#include "common.h"
#include "mlp_layout.h"

#define BANDS_BLOCK 256
#define BANDS_VIEW_PE 27

namespace {

struct BandRegions {
  int64_t l0, l5, vw, n_params;   // first float of LW[0], LW[5], VW; floats of the net
  int in_pe;
};

inline BandRegions band_regions(int kind) {
  const fnl::NetLayout& L = fnl::layout_of(kind);
  return BandRegions{L.LW[0], L.LW[5], L.VW, L.n_params, L.in_pe};
}

// whether element e of a net lies in one of the three regions; its weight in *w then
__device__ __forceinline__ bool band_weight(const BandRegions& R, const float* w_pos, const float* w_view, int64_t e, float* w) {
  const int64_t a = e - R.l0, b = e - R.l5, c = e - R.vw;
  if (a >= 0 && a < (int64_t)256 * R.in_pe) {
    *w = w_pos[(int)(a % R.in_pe)];
    return true;
  }
  if (b >= 0 && b < (int64_t)256 * (256 + R.in_pe)) {
    const int col = (int)(b % (256 + R.in_pe));
    if (col < R.in_pe) *w = w_pos[col];
    return col < R.in_pe;
  }
  if (c >= 0 && c < (int64_t)128 * (256 + BANDS_VIEW_PE)) {
    const int col = (int)(c % (256 + BANDS_VIEW_PE));
    if (col >= 256) *w = w_view[col - 256];
    return col >= 256;
  }
  return false;
}

__global__ void __launch_bounds__(BANDS_BLOCK) band_apply_kernel(BandRegions R, const float* w_pos, const float* w_view, const float* master,
                                                                 float* effective) {
  const int64_t stride = (int64_t)gridDim.x * BANDS_BLOCK;
  for (int64_t e = (int64_t)blockIdx.x * BANDS_BLOCK + threadIdx.x; e < R.n_params; e += stride) {
    float w = 1.f;
    const float x = master[e];
    effective[e] = band_weight(R, w_pos, w_view, e, &w) ? fmul(x, w) : x;
  }
}

// element i of the three regions laid end to end -> its float in the net and its weight
__global__ void __launch_bounds__(BANDS_BLOCK) band_grad_kernel(BandRegions R, const float* w_pos, const float* w_view, float* grads) {
  const int64_t n0 = (int64_t)256 * R.in_pe, total = 2 * n0 + (int64_t)128 * BANDS_VIEW_PE;
  const int64_t stride = (int64_t)gridDim.x * BANDS_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * BANDS_BLOCK + threadIdx.x; i < total; i += stride) {
    int64_t e;
    float w;
    if (i < n0) {
      e = R.l0 + i;
      w = w_pos[(int)(i % R.in_pe)];
    } else if (i < 2 * n0) {
      const int64_t j = i - n0;
      const int col = (int)(j % R.in_pe);
      e = R.l5 + (j / R.in_pe) * (256 + R.in_pe) + col;
      w = w_pos[col];
    } else {
      const int64_t j = i - 2 * n0;
      const int col = (int)(j % BANDS_VIEW_PE);
      e = R.vw + (j / BANDS_VIEW_PE) * (256 + BANDS_VIEW_PE) + 256 + col;
      w = w_view[col];
    }
    grads[e] = fmul(grads[e], w);
  }
}

inline unsigned bands_grid(int64_t n) {
  const int64_t blocks = (n + BANDS_BLOCK - 1) / BANDS_BLOCK;
  return (unsigned)(blocks < 2048 ? blocks : 2048);      // 256 CUs x 8: a few floats per lane of the 595844
}

}  // namespace

extern "C" int fastnerf_band_apply(int kind, const float* w_pos, const float* w_view, const float* master, float* effective,
                                   fn_stream_t stream) {
  FN_CHECK_ARG(kind >= 0 && kind <= 2, "kind in 0..2");
  FN_CHECK_ARG(w_pos && w_view && master && effective, "non-null pointers");
  FN_CHECK_ARG(master != effective, "master and effective are two buffers");
  const BandRegions R = band_regions(kind);
  hipLaunchKernelGGL(band_apply_kernel, dim3(bands_grid(R.n_params)), dim3(BANDS_BLOCK), 0, fn::S(stream), R, w_pos, w_view, master,
                     effective);
  FN_LAUNCH_CHECK();
  return 0;
}

extern "C" int fastnerf_band_grad(int kind, const float* w_pos, const float* w_view, float* grads, fn_stream_t stream) {
  FN_CHECK_ARG(kind >= 0 && kind <= 2, "kind in 0..2");
  FN_CHECK_ARG(w_pos && w_view && grads, "non-null pointers");
  const BandRegions R = band_regions(kind);
  hipLaunchKernelGGL(band_grad_kernel, dim3(bands_grid(2 * (int64_t)256 * R.in_pe + 128 * BANDS_VIEW_PE)), dim3(BANDS_BLOCK), 0,
                     fn::S(stream), R, w_pos, w_view, grads);
  FN_LAUNCH_CHECK();
  return 0;
}
