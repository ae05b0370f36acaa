// mlp_layout.h -- parameter / packed-weight / activation layouts of the 8x256 MLPs on the hot path.
//
// kind 0: NeRF            (nerf-ours/model.py:8-63,     input PE 63, parameters() order
//                          pts_linears.*, views_linears.0, feature_linear, alpha_linear, rgb_linear)
// kind 1: MLPNet fg       (nerf++-ours/nerf_network.py:70-142, input PE 63, order base_layers.*,
//                          sigma_layers.0, base_remap_layers.0, rgb_layers.0, rgb_layers.2)
// kind 2: MLPNet bg       (same, input PE 84 = 4-D inverted-sphere point)
// All three share the structure  L0..L7 (skip into L5) -> {sigma/alpha, remap/feature} -> view layer -> rgb.
#pragma once
#include <stdint.h>

namespace fnl {
struct NetLayout {
  int64_t LW[8], LB[8];                    // trunk weights / biases (flat offsets, [out][in] row-major)
  int64_t VW, VB, FW, FB, AW, AB, RW, RB;  // view layer, feature/remap, alpha/sigma, rgb
  int64_t PF[10], PB[9];                   // packed (fragment order) offsets: fwd L0..L7,F,V ; bwd Vt,Ft,L7t..L1t (F, V, Vt, Ft: unfused, no kernel reads them)
  // the folded view layer (feature / remap layer multiplied into the view layer's first 256 columns: M = Wv[:, :256] Wf, b' = bv + Wv[:, :256] bf).
  // Both packed buffers carry their part as appended regions, so a packed buffer is plain data (a copy of it is as good as the original):
  // PBM = M^T in the order of PB[0], behind PB[8] in the backward buffer; behind PF[9] in the forward buffer PFM = [M | Wv[:, 256:]] in the
  // view layer's forward order, PFB = b' (128 plain floats), PFR = M as plain row-major fp32 [128][256] (what the two packings are made from).
  // PFB / PFR hold plain floats in every math mode: `fold_plain` gives their float offset in a buffer of that mode.  fold_total = the size of
  // PFM | PFB | PFR, the tail of pf_total (host only; it keeps its place: the kernels load the members behind it by their offset).
  int64_t PFM, PFB, PFR, PBM, fold_total;
  int64_t n_params, pf_total, pb_total;
  int in_pe, pe_pad;                       // 63 -> 64, 84 -> 96
  int kind;
};

inline NetLayout make_layout(int kind) {
  NetLayout L{};
  L.kind = kind;
  L.in_pe = (kind == 2) ? 84 : 63;
  L.pe_pad = (kind == 2) ? 96 : 64;
  int64_t o = 0;
  for (int i = 0; i < 8; ++i) {
    const int fan = (i == 0) ? L.in_pe : (i == 5 ? 256 + L.in_pe : 256);
    L.LW[i] = o; o += (int64_t)256 * fan;
    L.LB[i] = o; o += 256;
  }
  auto V = [&]() { L.VW = o; o += 128 * 283; L.VB = o; o += 128; };
  auto F = [&]() { L.FW = o; o += 256 * 256; L.FB = o; o += 256; };
  auto A = [&]() { L.AW = o; o += 256; L.AB = o; o += 1; };
  auto R = [&]() { L.RW = o; o += 3 * 128; L.RB = o; o += 3; };
  if (kind == 0) { V(); F(); A(); R(); } else { A(); F(); V(); R(); }
  L.n_params = o;
  int64_t p = 0;
  for (int l = 0; l < 10; ++l) {
    L.PF[l] = p;
    const int kp = (l == 0) ? L.pe_pad : (l == 5 ? L.pe_pad + 256 : (l == 9 ? 288 : 256));
    p += (int64_t)kp * (l == 9 ? 128 : 256);
  }
  L.PFM = p; p += (int64_t)288 * 128;
  L.PFB = p; p += 128;
  L.PFR = p; p += (int64_t)128 * 256;
  L.fold_total = p - L.PFM;
  L.pf_total = p;
  p = 0;
  for (int j = 0; j < 9; ++j) { L.PB[j] = p; p += (int64_t)(j == 0 ? 128 : 256) * 256; }
  L.PBM = p; p += (int64_t)128 * 256;
  L.pb_total = p;
  return L;
}
// the three layouts, made once (kind out of range: kind 0; the entry points check it first)
inline const NetLayout& layout_of(int kind) {
  static const NetLayout L[3] = {make_layout(0), make_layout(1), make_layout(2)};
  return L[kind < 0 || kind > 2 ? 0 : kind];
}

// float offset of a plain-float region (PFB, PFR) in a packed buffer: the bf16x6 packing holds 3/2 floats per unit of the offsets above
inline __host__ __device__ int64_t fold_plain(int64_t off, bool x6) { return x6 ? off * 3 / 2 : off; }

// ---- saved activations, SoA over P points: pe | h0..h7 | (feat: a hole since the fold, nothing reads or writes it) | vpe32 | hv128 | ReLU sign words ----
constexpr int ACT_REST = 8 * 256 + 256 + 32 + 128;   // 2464 floats per point after the pe block
constexpr int ACT_MASK = 64;                         // 256 bytes of sign words per point (one 64-bit word per lane, layer and wave: mlp_common.h epilogue_fwd)
inline __host__ __device__ int64_t act_pe(int64_t P, int pe_pad) { return 0; }
inline __host__ __device__ int64_t act_h(int64_t P, int pe_pad, int l) { return P * pe_pad + (int64_t)l * P * 256; }
inline __host__ __device__ int64_t act_feat(int64_t P, int pe_pad) { return P * (pe_pad + 2048); }
inline __host__ __device__ int64_t act_vpe(int64_t P, int pe_pad) { return P * (pe_pad + 2048 + 256); }
inline __host__ __device__ int64_t act_hv(int64_t P, int pe_pad) { return P * (pe_pad + 2048 + 256 + 32); }
inline __host__ __device__ int64_t act_mask(int64_t P, int pe_pad) { return P * (pe_pad + ACT_REST); }  // uint64 words
inline int64_t act_floats(int64_t P, int pe_pad) { return P * (pe_pad + ACT_REST + ACT_MASK) + 8192; }
// ---- pre-activation gradients, SoA (dact_feat: a hole since the fold) ----
constexpr int DACT_FLOATS = 8 * 256 + 256 + 128;
inline __host__ __device__ int64_t dact_y(int64_t P, int l) { return (int64_t)l * P * 256; }
inline __host__ __device__ int64_t dact_feat(int64_t P) { return 8 * P * 256; }
inline __host__ __device__ int64_t dact_yv(int64_t P) { return 9 * P * 256; }
}  // namespace fnl
