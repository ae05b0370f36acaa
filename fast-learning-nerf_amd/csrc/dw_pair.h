// dw_pair.h -- plain structures shared by mlp_bwd_dw.hip (which fills and launches them), mlp_bf16.hip (the dW job table) and render.cpp
// (which holds the two DwDeferred of a paired backward on its stack): the dW jobs of a net and their partial regions, the job table of a
// trunk launch, the segment table of reduce_all, and what a pass of the paired bf16x6 backward leaves undone.  No HIP types here.
#pragma once
#include <stdint.h>

// dW jobs of one net (mlp_bwd_dw.hip and mlp_bf16.hip): NO, KI, bias?, rank1?   (KI of the two pe jobs = the layout's pe_pad)
struct DwJobDesc { int NO, KI, bias, rank1; };
inline DwJobDesc dw_job(int j, int pe_pad) {
  switch (j) {
    case 0: return {256, pe_pad, 1, 0};     // L0 (pe)
    case 8: return {256, pe_pad, 0, 0};     // L5 (pe part)
    case 9: return {256, 256, 1, 1};        // bf16x3: feature / remap layer (+ alpha / sigma row).  fp32 / bf16x6 (the layer is folded): its region holds the view job's rank-1 partials and G
    case 10: return {128, 256, 1, 0};       // view layer (h7 part: G = dL/dM; bf16x3: feature part)
    case 11: return {128, 32, 0, 0};        // view layer (vpe part)
    default: return {256, 256, 1, 0};       // 1..7: L1..L7 (h part)
  }
}
#define HEAD_MAX_WG 1024
inline int64_t dw_job_floats(int j, int pe_pad) {
  const DwJobDesc d = dw_job(j, pe_pad);
  return (int64_t)d.NO * d.KI + (d.bias ? d.NO : 0) + (d.rank1 ? d.KI : 0);
}
// regions in the order 0, 8, 1..7, 9, 10, 11 (then the head partials, "job 12"): the pairs that the bf16x6 path runs as ONE job
// (0 + 8: both multiply the positional encoding; 10 + 11: both multiply dYv) are neighbours
inline int64_t dw_job_base(int j, int ncu, int pe_pad) {
  static const int order[12] = {0, 8, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11};
  int64_t o = 0;
  for (int i = 0; i < 12; ++i) {
    if (order[i] == j) return o;
    o += dw_job_floats(order[i], pe_pad) * ncu;
  }
  return o;   // j == 12: everything
}
// floats of a net's partial buffer on a part with `ncu` CUs, sized for the widest layout (both *_partial_floats exports)
inline int64_t dw_partial_floats(int ncu) { return dw_job_base(12, ncu, 96) + (int64_t)HEAD_MAX_WG * 388; }

// ---- the rebuilding view job (bf16x6, 64-channel encoding, plain backward; mlp_bwd_dw.hip) ------------------------------------
// The view job of a pass can form dYv, the gradient at the view layer's pre-activation, on chip from (hv, draw, Wr) instead of reading what dX
// stored: 512 bytes a point that are then neither written nor read.  A caller whose call lets nothing else read dact_yv (the fused step,
// render.cpp) asks for it with a SideRb:
#define FN_DX_NO_DYV_STORE 1        // mlp_bwd_dx_kernel `flags`: dact_yv is not written
struct SideRb {
  int no_store;          // dX shall not store dYv
  int poison;            // FASTNERF_SIDE_REBUILD=nan: dact_yv is filled with NaNs before the backward's first kernel
};

#define DW_TRUNK_JOBS 7
struct DwTrunk {
  const float* dY[DW_TRUNK_JOBS];
  const float* X[DW_TRUNK_JOBS];
  float* pw[DW_TRUNK_JOBS];
  float* pb[DW_TRUNK_JOBS];
};

// ---- one launch reduces every job's per-workgroup partials into the flat gradient ------------
struct RedSeg {
  int64_t src;        // offset into the partial buffer
  int64_t wg_stride;  // floats between consecutive workgroups' partials
  int64_t dst;        // offset into the flat gradient
  int nwg, rows, cols, ld, valid_cols;
  int dyn;            // 1: the segment's chunk count is dw_trunk_chunks(point count) (the trunk launch), 2: head_rows(point count) (the head partials grouped from dX's tiles); nwg is its capacity
  int sc_cols;        // > 0: columns < sc_cols do not go to the gradient but to scratch[sc_dst + r * sc_cols + c] (G = dL/dM of the folded view layer)
  int64_t sc_dst;
};
#define MAX_SEGS 32
struct RedTable {
  RedSeg s[MAX_SEGS];
  int n;
};

// What a pass of the paired bf16x6 backward leaves undone (bwd_launch_t with `defer`): its trunk jobs, which fn::x6_pair_finish launches together
// with the other pass's, and its reduction + unfold, which follow that launch.
struct DwDeferred {
  DwTrunk J;
  RedTable T;
  int64_t P, g_off;
  const float* params;
  float *partial, *grads;
  int kind;
};
