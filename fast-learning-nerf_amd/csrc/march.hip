// march.hip -- fastnerf_occ_march (include/fastnerf.h, "marched render"): the placement kernel of the render that marches the occupancy
// grid, for gfx950.  Per ray a fixed lattice of K depths (coarse_depth of depths.h: the bits of fastnerf_sample_coarse with S = K) is walked,
// the lattice points whose lookup (occ_point of occ_lookup.h at x = o + d * z_k, through one grid or a cascade) says occupied are
// kept, and each maximal run of them is stored in the ray's packed row of C slots, followed by one closing entry that gives the
// run's last sample the width it has in the dense pass.  tests/march_numpy.py restates the kernel operation for operation.
//
// One thread per ray, 256 per block, no LDS, no atomics, plain vector stores; the bit words come through the cache (128^3 cells are
// 256 KB).  A ray's 44 bytes are read once per round.  Lanes diverge -- each ray has its own runs -- so the loop body is kept to one
// shape: a group of MARCH_GROUP lattice points is looked up at once (their loads are independent and in flight together), then the
// group's bits are consumed one lattice point per iteration with a store under a predicate.  What a round looked up and did not
// consume (the segment ended inside a group) travels in the ray's state to the next round, so a ray makes at most K lookups over
// all rounds (K + MARCH_GROUP - 1 counting the clamped repeats of lattice point K - 1 in the last group, whose answers are dropped).
//
// Bounds.  The host checks 2 <= K < 2^24, 2 <= C <= 512, 0 <= s0 < s1 <= C and n * C < 2^31.  Every iteration of the walk consumes
// one lattice point, so a round ends after at most K iterations whatever the lookups answer; the overflow scan advances by a whole
// group per iteration.  A store goes to slot s with s0 <= s < s1, or to slot s1 when s1 < C (the depth that fastnerf_ert_advance
// reads for the width of slot s1 - 1): at most s1 - s0 + 1 slots, every index < C.  A state that the caller's scratch does not hold
// (no first round) is clamped into 0 <= k <= K, k + leftover <= K before it is used.  Non-finite rays and near >= far take the same
// path: their points fall outside every box and take `outside`.
//
// fastnerf_occ_march_jitter (include/fastnerf.h, "marched training") walks the same lattice shifted per ray by u_r in [0, 1):
// z_k(u) = z_k + u_r (z_{k+1} - z_k), k < K, and z_K(u) = z_{K-1}(u) + (z_K - z_{K-1}).  The walk is one template; what differs is the
// depth policy (NoShift / Shift below), so the instantiations of fastnerf_occ_march hold no branch on it.  fastnerf_march_mask zeroes the
// colour gradient of the rays whose row overflowed.
#include "common.h"
#include "depths.h"
#include "occ_lookup.h"

#define MARCH_BLOCK 256
#define MARCH_GROUP 4   // lattice points looked up per batch; the leftover (< MARCH_GROUP bits, its count) fits bits 1..5 of the state

namespace {

struct MarchArgs {
  int64_t n;
  int K, lindisp, C, s0, s1, first;
  const float* rays;
  const float* trans;
  float eps;
  int32_t* state;
  float* z;
  int32_t* kidx;
  uint8_t* overflow;
};

// z_k, k = 0 .. K; z_K = z_{K-1} + (z_{K-1} - z_{K-2}) closes the last lattice point
__device__ __forceinline__ float lattice_z(float near, float far, int k, int K, int lindisp) {
  if (k < K) return coarse_depth(near, far, k, K, lindisp);
  const float a = coarse_depth(near, far, K - 1, K, lindisp), b = coarse_depth(near, far, K - 2, K, lindisp);
  return fadd(a, fsub(a, b));
}

// The depth policy of a walk.  u(r): the ray's shift, read once; point(k): the depth of lattice point k < K; any(k): k <= K.
struct NoShift {
  __device__ __forceinline__ float u(int64_t) const { return 0.f; }
  static __device__ __forceinline__ float point(float near, float far, int k, int K, int lindisp, float) {
    return coarse_depth(near, far, k, K, lindisp);
  }
  static __device__ __forceinline__ float any(float near, float far, int k, int K, int lindisp, float) {
    return lattice_z(near, far, k, K, lindisp);
  }
};

// u_r from the caller's buffer, or u01 of word 0 of Philox block r of the stream 'mrch' ("Random streams")
struct Shift {
  const float* ubuf;
  uint64_t seed;
  __device__ __forceinline__ float u(int64_t r) const {
    if (ubuf) return ubuf[r];
    uint32_t o[4];
    philox4x32((uint32_t)r, (uint32_t)((uint64_t)r >> 32), 0x6d726368u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), o);
    return u01(o[0]);
  }
  static __device__ __forceinline__ float point(float near, float far, int k, int K, int lindisp, float u) {
    const float zk = coarse_depth(near, far, k, K, lindisp);
    return fadd(zk, fmul(u, fsub(lattice_z(near, far, k + 1, K, lindisp), zk)));
  }
  static __device__ __forceinline__ float any(float near, float far, int k, int K, int lindisp, float u) {
    if (k < K) return point(near, far, k, K, lindisp, u);
    return fadd(point(near, far, K - 1, K, lindisp, u),
                fsub(lattice_z(near, far, K, K, lindisp), coarse_depth(near, far, K - 1, K, lindisp)));
  }
};

// bit j: lattice point k + j (< K) is live.  The points beyond K - 1 repeat K - 1 and are masked out: MARCH_GROUP independent lookups
template <class J, class G>
__device__ __forceinline__ unsigned march_group(const G& g, const float* o, const float* d, float near, float far, int k, int K, int lindisp,
                                                float u) {
  // occ_point, split (occ_lookup.h): the index arithmetic of all the points first, then their loads -- unconditional, a point outside
  // every box reads bit 0 of the first grid and drops it -- so that the loads are issued back to back and waited for once
  const uint32_t* words[MARCH_GROUP];
  uint32_t cell[MARCH_GROUP];
  bool inside[MARCH_GROUP];
#pragma unroll
  for (int j = 0; j < MARCH_GROUP; ++j) {
    const int kk = k + j < K ? k + j : K - 1;
    const float zz = J::point(near, far, kk, K, lindisp, u);
    inside[j] = occ_locate(g, fadd(o[0], fmul(d[0], zz)), fadd(o[1], fmul(d[1], zz)), fadd(o[2], fmul(d[2], zz)), words[j], cell[j]);
  }
  uint32_t w[MARCH_GROUP];
#pragma unroll
  for (int j = 0; j < MARCH_GROUP; ++j) w[j] = words[j][cell[j] >> 5];
  unsigned m = 0;
#pragma unroll
  for (int j = 0; j < MARCH_GROUP; ++j) {
    const bool b = inside[j] ? ((w[j] >> (cell[j] & 31u)) & 1u) != 0u : occ_outside(g) != 0;
    if (b && k + j < K) m |= 1u << j;
  }
  return m;
}

template <class G, class J>
__global__ void __launch_bounds__(MARCH_BLOCK) occ_march_kernel(G g, MarchArgs a, J jit) {
  const int64_t r = (int64_t)blockIdx.x * MARCH_BLOCK + threadIdx.x;
  if (r >= a.n) return;
  const float* rr = a.rays + r * 11;
  const float o[3] = {rr[0], rr[1], rr[2]}, d[3] = {rr[3], rr[4], rr[5]};
  const float near = rr[6], far = rr[7];
  const int K = a.K, C = a.C;
  const float u = jit.u(r);
  // the state: the next lattice index, whether slot s0 - 1 holds a live sample (its closing depth is owed), and the leftover lookups
  int k = 0, nv = 0;
  unsigned m = 0;
  bool pend = false;
  if (!a.first) {
    k = a.state[r * 2];
    const int st = a.state[r * 2 + 1];
    k = k < 0 ? 0 : (k > K ? K : k);
    pend = st & 1;
    nv = (st >> 4) & 3;
    nv = nv < K - k ? nv : K - k;
    m = ((unsigned)st >> 1) & ((1u << nv) - 1u);
  }
  float* zr = a.z + r * C;
  int32_t* kr = a.kidx + r * C;
  int s = a.s0;
  float zlast = a.s0 > 0 ? zr[a.s0 - 1] : J::any(near, far, 0, K, a.lindisp, u);
  bool ovf = false;
  if (a.trans && !(a.trans[r] > a.eps)) {
    // cut: the lattice position stays; a live slot s0 - 1 still gets its closing entry, everything else is padding
    if (pend) {
      zlast = J::any(near, far, k, K, a.lindisp, u);
      zr[s] = zlast;
      kr[s] = -1;
      ++s;
      pend = false;
    }
  } else {
    while (s < a.s1) {
      if (nv == 0) {
        if (k >= K) break;
        m = march_group<J>(g, o, d, near, far, k, K, a.lindisp, u);
        nv = K - k < MARCH_GROUP ? K - k : MARCH_GROUP;
      }
      const bool lv = m & 1u;
      m >>= 1;
      --nv;
      if (lv || pend) {   // a live sample, or the closing entry of the run that ended at k - 1
        const bool last = s == C - 1;   // slot C - 1 never holds a live sample: the sequence goes on behind it
        zlast = J::point(near, far, k, K, a.lindisp, u);
        zr[s] = zlast;
        kr[s] = (lv && !last) ? k : -1;
        ovf = ovf || (lv && last);
        ++s;
        pend = lv && !last;
      }
      ++k;
    }
    if (s < a.s1 && pend) {   // the lattice ended inside a run: lattice point K - 1 is closed at z_K
      zlast = J::any(near, far, K, K, a.lindisp, u);
      zr[s] = zlast;
      kr[s] = -1;
      ++s;
      pend = false;
    }
    if (s == C) {   // a full row: it overflows when a live lattice point is left
      while (!ovf) {
        if (nv == 0) {
          if (k >= K) break;
          m = march_group<J>(g, o, d, near, far, k, K, a.lindisp, u);
          nv = K - k < MARCH_GROUP ? K - k : MARCH_GROUP;
        }
        ovf = m != 0u;
        k += nv;
        nv = 0;
        m = 0;
      }
      k = K;
      nv = 0;
      m = 0;
    }
  }
  for (; s < a.s1; ++s) {
    zr[s] = zlast;
    kr[s] = -1;
  }
  if (a.s1 < C) zr[a.s1] = pend ? J::any(near, far, k, K, a.lindisp, u) : zlast;   // in place before the segment's advance runs
  a.state[r * 2] = k;
  a.state[r * 2 + 1] = (int)((pend ? 1u : 0u) | (m << 1) | ((unsigned)nv << 4));
  if (a.first) a.overflow[r] = ovf ? 1 : 0;
  else if (ovf) a.overflow[r] = 1;
}

template <class G, class J>
void march_launch(const G& g, const MarchArgs& a, const J& jit, hipStream_t s) {
  hipLaunchKernelGGL((occ_march_kernel<G, J>), dim3((unsigned)((a.n + MARCH_BLOCK - 1) / MARCH_BLOCK)), dim3(MARCH_BLOCK), 0, s, g, a, jit);
}

__global__ void __launch_bounds__(MARCH_BLOCK) march_mask_kernel(int64_t n, const uint8_t* overflow, float* g_rgb) {
  const int64_t r = (int64_t)blockIdx.x * MARCH_BLOCK + threadIdx.x;
  if (r >= n || !overflow[r]) return;
  g_rgb[r * 3] = 0.f;
  g_rgb[r * 3 + 1] = 0.f;
  g_rgb[r * 3 + 2] = 0.f;
}

}  // namespace

extern "C" int fastnerf_occ_march(const fn_occ_grid* grid, const fn_occ_cascade* cascade, int64_t n, int K, int lindisp, const float* rays11,
                                  int C, int s0, int s1, int first, const float* trans, float eps, int32_t* state, float* z, int32_t* kidx,
                                  uint8_t* overflow, fn_stream_t stream) {
  OccDev g;
  OccCascadeDev c;
  FN_CHECK_ARG((grid != nullptr) != (cascade != nullptr), "exactly one of grid / cascade");
  FN_CHECK_ARG(!grid || occ_dev(grid, &g), OCC_GRID_ARG);
  FN_CHECK_ARG(!cascade || occ_cascade_dev(cascade, &c), OCC_CASCADE_ARG);
  FN_CHECK_ARG(n >= 0 && K >= 2 && K < (1 << 24) && C >= 2 && C <= 512 && n * (int64_t)C < ((int64_t)1 << 31),
               "n >= 0, 2 <= K < 2^24, 2 <= C <= 512, n * C < 2^31");
  FN_CHECK_ARG(s0 >= 0 && s0 < s1 && s1 <= C && (first != 0) == (s0 == 0), "0 <= s0 < s1 <= C, first exactly when s0 == 0");
  FN_CHECK_ARG(!trans || (eps >= 0.f && eps < 1.f), "0 <= eps < 1");
  if (n == 0) return 0;
  FN_CHECK_ARG(rays11 && state && z && kidx && overflow, "non-null pointers");
  const MarchArgs a = {n, K, lindisp ? 1 : 0, C, s0, s1, first ? 1 : 0, rays11, trans, eps, state, z, kidx, overflow};
  if (grid) march_launch(g, a, NoShift{}, fn::S(stream));
  else march_launch(c, a, NoShift{}, fn::S(stream));
  FN_LAUNCH_CHECK();
  return 0;
}

extern "C" int fastnerf_occ_march_jitter(const fn_occ_grid* grid, const fn_occ_cascade* cascade, int64_t n, int K, int lindisp,
                                         const float* rays11, int C, int s0, int s1, int first, const float* trans, float eps,
                                         const float* u, uint64_t seed, int32_t* state, float* z, int32_t* kidx, uint8_t* overflow,
                                         fn_stream_t stream) {
  // no shift: the launch of fastnerf_occ_march itself
  if (!u && seed == 0) return fastnerf_occ_march(grid, cascade, n, K, lindisp, rays11, C, s0, s1, first, trans, eps, state, z, kidx, overflow, stream);
  OccDev g;
  OccCascadeDev c;
  FN_CHECK_ARG((grid != nullptr) != (cascade != nullptr), "exactly one of grid / cascade");
  FN_CHECK_ARG(!grid || occ_dev(grid, &g), OCC_GRID_ARG);
  FN_CHECK_ARG(!cascade || occ_cascade_dev(cascade, &c), OCC_CASCADE_ARG);
  FN_CHECK_ARG(n >= 0 && K >= 2 && K < (1 << 24) && C >= 2 && C <= 512 && n * (int64_t)C < ((int64_t)1 << 31),
               "n >= 0, 2 <= K < 2^24, 2 <= C <= 512, n * C < 2^31");
  FN_CHECK_ARG(s0 >= 0 && s0 < s1 && s1 <= C && (first != 0) == (s0 == 0), "0 <= s0 < s1 <= C, first exactly when s0 == 0");
  FN_CHECK_ARG(!trans || (eps >= 0.f && eps < 1.f), "0 <= eps < 1");
  if (n == 0) return 0;
  FN_CHECK_ARG(rays11 && state && z && kidx && overflow, "non-null pointers");
  const MarchArgs a = {n, K, lindisp ? 1 : 0, C, s0, s1, first ? 1 : 0, rays11, trans, eps, state, z, kidx, overflow};
  const Shift j = {u, seed};
  if (grid) march_launch(g, a, j, fn::S(stream));
  else march_launch(c, a, j, fn::S(stream));
  FN_LAUNCH_CHECK();
  return 0;
}

// g_rgb [n,3]: the rows of the rays with overflow[r] != 0 are zeroed, every other row keeps its bits
extern "C" int fastnerf_march_mask(int64_t n, const uint8_t* overflow, float* g_rgb, fn_stream_t stream) {
  FN_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31), "0 <= n < 2^31");
  if (n == 0) return 0;
  FN_CHECK_ARG(overflow && g_rgb, "non-null pointers");
  hipLaunchKernelGGL(march_mask_kernel, dim3((unsigned)((n + MARCH_BLOCK - 1) / MARCH_BLOCK)), dim3(MARCH_BLOCK), 0, fn::S(stream), n,
                     overflow, g_rgb);
  FN_LAUNCH_CHECK();
  return 0;
}
