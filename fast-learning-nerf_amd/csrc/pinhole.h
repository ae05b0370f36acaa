// pinhole.h -- the pinhole camera of get_rays (run_nerf_helpers.py:68-78), shared by the ray generators (rays.hip) and the pose
// gradient (pose.hip): one statement of the arithmetic, so that a ray rebuilt from its pixel is the ray that was generated.
#pragma once
#include "common.h"

// dir = ((col - cx) / fx, -(row - cy) / fy, -1): the pixel's direction in camera axes
__device__ __forceinline__ void pixel_dir(float row, float col, float fx, float fy, float cx, float cy, float dir[3]) {
  dir[0] = (col - cx) / fx;
  dir[1] = -(row - cy) / fy;
  dir[2] = -1.0f;
}

// d = R dir with the rotation of the row-major 3x4 pose c
__device__ __forceinline__ void rotate_dir(const float dir[3], const float* __restrict__ c, float d[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k)
    d[k] = fadd(fadd(fmul(dir[0], c[4 * k + 0]), fmul(dir[1], c[4 * k + 1])), fmul(dir[2], c[4 * k + 2]));
}

__device__ __forceinline__ void pixel_ray(float row, float col, float fx, float fy, float cx, float cy,
                                          const float* __restrict__ c, float d[3]) {
  float dir[3];
  pixel_dir(row, col, fx, fy, cx, cy, dir);
  rotate_dir(dir, c, d);
}
