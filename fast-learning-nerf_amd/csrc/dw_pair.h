// dw_pair.h -- plain structures shared by mlp_bwd_dw.hip (which fills and launches them) and render.cpp (which holds the two DwDeferred
// of a paired backward on its stack): the job table of a trunk launch, the segment table of reduce_all, and what a pass of the paired
// bf16x6 backward leaves undone.  No HIP types here.
#pragma once
#include <stdint.h>

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
