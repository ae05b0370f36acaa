// seg_reduce.h -- what the segmented per-image sums share (pose.hip: fastnerf_pose_grad, exposure.hip: fastnerf_expo_grad): the rule that
// cuts a batch into chunks, and the fixed tree in which the 256 lane sums of a workgroup meet.  Workgroup (img, c) walks chunk c of the
// batch -- a contiguous range of rays, C chunks, C a function of (n, n_img) alone -- lane t takes rays t, t + 256, ... of the chunk in
// order, and a second launch adds an image's C partial sums in chunk order.  Which lane and which chunk a ray falls to depends on its row
// index alone: no atomics, bit-identical from call to call.
#pragma once
#include "common.h"

#define FN_SEG_BLOCK 256
#define FN_SEG_MIN_CHUNK 1024      // rays per workgroup below which splitting further only adds partial sums
#define FN_SEG_MAX_GROUPS 1024     // n_img * C stays near this: four workgroups per CU

static inline int seg_chunks(int64_t n, int n_img) {
  int64_t by_rays = (n + FN_SEG_MIN_CHUNK - 1) / FN_SEG_MIN_CHUNK;
  int64_t by_groups = FN_SEG_MAX_GROUPS / n_img;
  int64_t c = by_rays < by_groups ? by_rays : by_groups;
  return c < 1 ? 1 : (int)c;
}

__device__ __forceinline__ float seg_add(float a, float b) { return fadd(a, b); }
__device__ __forceinline__ int32_t seg_add(int32_t a, int32_t b) { return a + b; }

// 256 -> 4: a wave's 64 lane sums by shuffles (offsets 32, 16, ..., 1), lane 0 of wave w leaves them in part[w].  Every lane of the
// workgroup calls this; behind it (it ends in the barrier) any lane may read part.
template <class T, int K>
__device__ __forceinline__ void seg_wave_sums(T (&acc)[K], T (&part)[FN_SEG_BLOCK / 64][K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    T x = acc[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = seg_add(x, __shfl_down(x, off, 64));
    acc[k] = x;
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) part[wave][k] = acc[k];
  }
  __syncthreads();
}

// 4 -> 1: element k of the workgroup's sum, the waves in wave order
template <class T, int K>
__device__ __forceinline__ T seg_total(const T (&part)[FN_SEG_BLOCK / 64][K], int k) {
  T x = part[0][k];
#pragma unroll
  for (int w = 1; w < FN_SEG_BLOCK / 64; ++w) x = seg_add(x, part[w][k]);
  return x;
}
