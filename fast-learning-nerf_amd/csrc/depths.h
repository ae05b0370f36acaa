// depths.h -- the unperturbed coarse depths of a ray (render.py:244-266), shared by the coarse sampler (rays.hip) and the lattice of
// the marched render (march.hip): one definition, hence one set of bits.
#pragma once
#include "common.h"

// torch.linspace(0,1,S) fp32: symmetric evaluation (start+step*i below the midpoint,
// end-step*(S-1-i) above it).
__device__ __forceinline__ float lin01(int i, int S) {
  const float step = 1.0f / (float)(S - 1);
  return (i < S / 2) ? fmul(step, (float)i) : fsub(1.0f, fmul(step, (float)(S - 1 - i)));
}

__device__ __forceinline__ float coarse_depth(float near, float far, int i, int S, int lindisp) {
  if (S == 1) return near;
  const float t = lin01(i, S);
  if (!lindisp) return fadd(fmul(near, fsub(1.0f, t)), fmul(far, t));
  return 1.0f / fadd(fmul(1.0f / near, fsub(1.0f, t)), fmul(1.0f / far, t));
}
