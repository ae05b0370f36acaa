// ray_bounds.hip -- fastnerf_occ_ray_bounds (include/fastnerf.h, "per-ray bounds from the occupancy grid"): per ray the part
// [near', far'] of [near, far] outside which the lookup of occupancy.hip (occ_point at x = o + d * z) cannot call a sample
// occupied, through one grid or a cascade, for gfx950.  tests/ray_bounds_numpy.py restates it operation for operation.
//
// One thread per ray, 256 per block, no LDS, no atomics, plain stores; the bit words are read through the cache (128^3 cells are
// 256 KB).  Lanes diverge -- the rays of a training batch are unrelated -- and a ray takes two short iterations per cell face it
// crosses; the loop has a hard cap that the host computes from the cell counts, so no input makes the kernel spin.
//
// The traversal.  Per level and axis the ray is og + dg * z in grid coordinates (og = (o - lo) * inv, dg = d * inv) and face k is
// crossed at t(k) = (k - og) / dg.  The lookup rounds differently (x = o + d * z first, then (x - lo) * inv), so ITS index along
// an axis changes somewhere in the window [t(k) - e, t(k) + e], e = delta / |dg|: delta = 2^-20 (B + n + 2) grid units, B =
// (|o| + |lo| + |d| max(|near|, |far|)) inv the magnitude of the terms, bounds the rounding of both chains (about 10 B 2^-24) with
// a factor to spare.  The lookup's index is monotone in z on every axis (each of its operations is), so at a depth z it is the last
// index the ray has SURELY reached (z >= t + e) or, inside a window, the next one.  The sweep walks the window starts and ends of
// the three axes in order of depth: between two events the lookup's cell is one of a block of 1, 2, 4 or 8 candidates, and the
// stretch counts as occupied when one of them is.  Nothing that fp32 rounding does at a face, an edge or a corner -- a ray in the
// plane of a face included, whose window is the whole ray -- can then put an occupied sample outside [near', far'], and the bounds
// are never more than e, far less than a cell, wider than the cells ask for.  A zero dg takes no step: its one or two candidates
// hold for the whole ray.
// A ray whose terms are too large for delta <= 1/4 (a camera 10^5 boxes away), like a non-finite one, one with near >= far and one
// that reaches the cap, keeps its bounds with hit = 1: unchanged bounds with hit = 1 are always a valid answer.
//
// A cascade is swept level by level.  A stretch that is occupied in level l counts unless the ray is SURELY inside the box of
// an earlier level there (from the end of the entry face's window to the start of the exit face's); with `outside_occupied` what
// is left of [near, far] after the stretches surely inside some box counts as well.  Only the first and the last occupied depth are
// kept, so a stretch is clipped against the (at most 7) earlier boxes only when it would move one of the two.  One grid is a
// cascade of one level: the same instructions, hence the same bits.
#include "common.h"

namespace fn {
const char* occ_cascade_fault(const fn_occ_cascade* c);   // occupancy.hip: NULL when every level is usable
}

#define RB_BLOCK 256
#define RB_ERR 9.5367431640625e-07f   // 2^-20
#define RB_DELTA_MAX 0.25f
#define RB_Z_LIMIT 1152921504606846976.f   // 2^60

namespace {

struct RbLevel {
  float lo[3], inv[3];
  int n[3];
  int pad;
};

struct RbDev {
  RbLevel g[FN_OCC_MAX_LEVELS];
  const uint32_t* words[FN_OCC_MAX_LEVELS];
  int levels;
  int outside;
  int cap;
};

// one axis of one level: the geometry, the stretches in which the lookup's index possibly / surely lies in 0 .. n-1, and the
// sweep's state: c = the last cell surely reached, amb = inside the window of the next face, tface = t(that face)
struct RbAxis {
  float og, dg, e, tnext, tface;
  float pin, pout, sin, sout;
  int n, c, s, step;
  bool amb;
};

__device__ __forceinline__ float rb_t(const RbAxis& x, int k) { return __fdiv_rn(fsub((float)k, x.og), x.dg); }
// (a NaN -- inf - inf with a huge e -- widens the window)
__device__ __forceinline__ float rb_win_start(const RbAxis& x, int k) {
  const float v = fsub(rb_t(x, k), x.e);
  return v == v ? v : -INFINITY;
}
__device__ __forceinline__ float rb_win_end(const RbAxis& x, int k) {
  const float v = fadd(rb_t(x, k), x.e);
  return v == v ? v : INFINITY;
}
__device__ __forceinline__ int rb_face(const RbAxis& x) { return x.s > 0 ? x.c + 1 : x.c; }

// false: the terms are too large for the error bound
__device__ __forceinline__ bool rb_axis(RbAxis& x, float o, float d, float lo, float inv, int n, float zmax) {
  x.n = n;
  x.og = fmul(fsub(o, lo), inv);
  x.dg = fmul(d, inv);
  const float B = fmul(fadd(fadd(fabsf(o), fabsf(lo)), fmul(fabsf(d), zmax)), inv);
  const float delta = fmul(RB_ERR, fadd(fadd(B, (float)n), 2.f));
  if (!(delta <= RB_DELTA_MAX)) return false;
  x.s = x.dg > 0.f ? 1 : (x.dg < 0.f ? -1 : 0);
  x.c = 0;
  x.amb = false;
  x.step = 1;
  x.tnext = INFINITY;
  x.tface = INFINITY;
  if (x.s) {
    x.e = __fdiv_rn(delta, fabsf(x.dg));
    const int kin = x.s > 0 ? 0 : n, kout = x.s > 0 ? n : 0;
    x.pin = rb_win_start(x, kin);
    x.pout = rb_win_end(x, kout);
    x.sin = rb_win_end(x, kin);
    x.sout = rb_win_start(x, kout);
  } else {
    x.e = INFINITY;
    const int c0 = (int)floorf(fsub(x.og, delta)), c1 = (int)floorf(fadd(x.og, delta));   // |og| <= B < 2^18
    x.c = c0;
    x.amb = c1 != c0;
    const bool possibly = c1 >= 0 && c0 <= n - 1, surely = c0 >= 0 && c1 <= n - 1;
    x.pin = possibly ? -INFINITY : INFINITY;
    x.pout = possibly ? INFINITY : -INFINITY;
    x.sin = surely ? -INFINITY : INFINITY;
    x.sout = surely ? INFINITY : -INFINITY;
  }
  return true;
}

// the state at depth z, inside the level's 'possibly inside' stretch; false: the estimate did not settle (keep the bounds)
__device__ __forceinline__ bool rb_start(RbAxis& x, float z) {
  if (!x.s) return true;   // c, amb hold for the whole ray
  x.step = x.s;
  const float est = floorf(fadd(x.og, fmul(x.dg, z)));
  x.c = est == est ? (int)fminf(fmaxf(est, -1.f), (float)x.n) : -1;
  bool ok = false;
  for (int i = 0; i < 4; ++i) {
    const int behind = x.s > 0 ? x.c : x.c + 1;
    const bool movable = x.s > 0 ? x.c > -1 : x.c < x.n;
    if (movable && rb_win_end(x, behind) > z) {
      x.c -= x.s;
    } else {
      ok = true;
      break;
    }
  }
  if (!ok) return false;
  ok = false;
  for (int i = 0; i < 4; ++i) {
    const bool movable = x.s > 0 ? x.c < x.n : x.c > -1;
    if (movable && rb_win_end(x, rb_face(x)) <= z) {
      x.c += x.s;
    } else {
      ok = true;
      break;
    }
  }
  if (!ok) return false;
  x.tface = rb_t(x, rb_face(x));
  x.amb = rb_win_start(x, rb_face(x)) <= z;
  x.tnext = x.amb ? rb_win_end(x, rb_face(x)) : rb_win_start(x, rb_face(x));
  return true;
}

// the next event of axis `am`: a window opens (the candidates grow by the next cell), or it closes (the cell is reached; one division
// per face).  ONE body for the three axes -- the state is selected in and out -- instead of three divergent ones.
__device__ __forceinline__ void rb_advance(int am, RbAxis& a0, RbAxis& a1, RbAxis& a2) {
  const float og = am == 0 ? a0.og : (am == 1 ? a1.og : a2.og), dg = am == 0 ? a0.dg : (am == 1 ? a1.dg : a2.dg);
  const float e = am == 0 ? a0.e : (am == 1 ? a1.e : a2.e);
  const int s = am == 0 ? a0.s : (am == 1 ? a1.s : a2.s);
  int c = am == 0 ? a0.c : (am == 1 ? a1.c : a2.c);
  bool amb = am == 0 ? a0.amb : (am == 1 ? a1.amb : a2.amb);
  float tface = am == 0 ? a0.tface : (am == 1 ? a1.tface : a2.tface), tnext;
  if (amb) {
    c += s;
    amb = false;
    tface = __fdiv_rn(fsub((float)(s > 0 ? c + 1 : c), og), dg);
    const float v = fsub(tface, e);
    tnext = v == v ? v : -INFINITY;
  } else {
    amb = true;
    const float v = fadd(tface, e);
    tnext = v == v ? v : INFINITY;
  }
#define RB_PUT(x, k)                        \
  x.c = am == k ? c : x.c;                  \
  x.amb = am == k ? amb : x.amb;            \
  x.tface = am == k ? tface : x.tface;      \
  x.tnext = am == k ? tnext : x.tnext;
  RB_PUT(a0, 0)
  RB_PUT(a1, 1)
  RB_PUT(a2, 2)
#undef RB_PUT
}

// one of the candidate cells that lie in the box has its bit set
__device__ __forceinline__ bool rb_any(const uint32_t* __restrict__ words, const RbAxis& a, const RbAxis& b, const RbAxis& c) {
  for (int p = 0; p <= (a.amb ? 1 : 0); ++p) {
    const int i = a.c + p * a.step;
    if ((unsigned)i >= (unsigned)a.n) continue;
    for (int q = 0; q <= (b.amb ? 1 : 0); ++q) {
      const int j = b.c + q * b.step;
      if ((unsigned)j >= (unsigned)b.n) continue;
      for (int r = 0; r <= (c.amb ? 1 : 0); ++r) {
        const int k = c.c + r * c.step;
        if ((unsigned)k >= (unsigned)c.n) continue;
        const uint32_t cell = ((uint32_t)i * (uint32_t)b.n + (uint32_t)j) * (uint32_t)c.n + (uint32_t)k;
        if ((words[cell >> 5] >> (cell & 31u)) & 1u) return true;
      }
    }
  }
  return false;
}

// first / last occupied depth so far, and the stretches surely inside the boxes of the levels swept so far
struct RbSpan {
  float lo, hi;
  float sin[FN_OCC_MAX_LEVELS], sout[FN_OCC_MAX_LEVELS];
};

// [ta, tb] is occupied in a level behind nl others: what is left of it outside their 'surely inside' stretches (whose end points
// stay) widens the span.  nl is uniform; the loops are unrolled so that sin / sout stay in registers.
__device__ __forceinline__ void rb_take(RbSpan& sp, float ta, float tb, int nl) {
  if (!(ta < sp.lo || tb > sp.hi)) return;
  float x = ta, y = tb;
#pragma unroll
  for (int p = 0; p < FN_OCC_MAX_LEVELS; ++p) {
    if (p >= nl) break;
#pragma unroll
    for (int j = 0; j < FN_OCC_MAX_LEVELS; ++j) {
      if (j < nl) {
        if (sp.sin[j] <= x && x <= sp.sout[j]) x = sp.sout[j];
        if (sp.sin[j] <= y && y <= sp.sout[j]) y = sp.sin[j];
      }
    }
  }
  if (x <= tb && y >= ta && x <= y) {
    sp.lo = fminf(sp.lo, x);
    sp.hi = fmaxf(sp.hi, y);
  }
}

// 0: no occupied stretch (hit = 0); 1: keep the bounds, hit = 1; 2: [*n2, *f2], hit = 1
__device__ __forceinline__ int rb_ray(const RbDev& c, const float* o, const float* d, float near, float far, float* n2, float* f2) {
  const bool finite = isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]) && isfinite(d[0]) && isfinite(d[1]) && isfinite(d[2]) &&
                      isfinite(near) && isfinite(far);
  if (!finite || !(near < far)) return 1;
  const float zmax = fmaxf(fabsf(near), fabsf(far));
  if (!(zmax <= RB_Z_LIMIT)) return 1;
  RbSpan sp;
  sp.lo = INFINITY;
  sp.hi = -INFINITY;
#pragma unroll
  for (int j = 0; j < FN_OCC_MAX_LEVELS; ++j) {
    sp.sin[j] = INFINITY;
    sp.sout[j] = -INFINITY;
  }
  int it = 0;
  for (int l = 0; l < c.levels; ++l) {   // (uniform: the level's geometry comes through scalar loads)
    const RbLevel& g = c.g[l];
    const uint32_t* __restrict__ words = c.words[l];
    RbAxis a0, a1, a2;
    if (!rb_axis(a0, o[0], d[0], g.lo[0], g.inv[0], g.n[0], zmax)) return 1;
    if (!rb_axis(a1, o[1], d[1], g.lo[1], g.inv[1], g.n[1], zmax)) return 1;
    if (!rb_axis(a2, o[2], d[2], g.lo[2], g.inv[2], g.n[2], zmax)) return 1;
    const float s0 = fmaxf(near, fmaxf(a0.pin, fmaxf(a1.pin, a2.pin)));
    const float s1 = fminf(far, fminf(a0.pout, fminf(a1.pout, a2.pout)));
    if (s0 <= s1) {
      if (!rb_start(a0, s0) || !rb_start(a1, s0) || !rb_start(a2, s0)) return 1;
      float tcur = s0;
      // the last test's result, while it says something about this stretch: the candidates of consecutive stretches differ by one
      // event -- a window that opened (a superset: true stays true) or closed (a subset: false stays false)
      bool known = false, prev = false, grew = false;
      for (;;) {
        if (++it > c.cap) return 1;
        int am = 0;
        float tn = a0.tnext;
        if (a1.tnext < tn) {
          am = 1;
          tn = a1.tnext;
        }
        if (a2.tnext < tn) {
          am = 2;
          tn = a2.tnext;
        }
        const float tend = fmaxf(fminf(tn, s1), tcur);
        if (tcur < sp.lo || tend > sp.hi) {
          const bool occ = (known && prev == grew) ? prev : rb_any(words, a0, a1, a2);
          known = true;
          prev = occ;
          if (occ) rb_take(sp, tcur, tend, l);
        } else {
          known = false;   // inside the span: nothing to find, nothing looked up
        }
        if (!(tn < s1)) break;
        grew = !(am == 0 ? a0.amb : (am == 1 ? a1.amb : a2.amb));
        rb_advance(am, a0, a1, a2);
        tcur = tend;
      }
    }
    const float sin = fmaxf(a0.sin, fmaxf(a1.sin, a2.sin)), sout = fminf(a0.sout, fminf(a1.sout, a2.sout));
#pragma unroll
    for (int j = 0; j < FN_OCC_MAX_LEVELS; ++j) {
      if (j == l) {
        sp.sin[j] = sin;
        sp.sout[j] = sout;
      }
    }
  }
  if (c.outside) rb_take(sp, near, far, c.levels);
  if (!(sp.lo <= sp.hi)) return 0;
  const float a = fmaxf(near, sp.lo), b = fminf(far, sp.hi);
  if (!(a < b)) return 1;
  *n2 = a;
  *f2 = b;
  return 2;
}

__global__ void __launch_bounds__(RB_BLOCK) ray_bounds_kernel(RbDev c, int64_t n, float* __restrict__ rays11, int write_back,
                                                              float* __restrict__ bounds, uint8_t* __restrict__ hit) {
  const int64_t q = (int64_t)blockIdx.x * RB_BLOCK + threadIdx.x;
  if (q >= n) return;
  float* row = rays11 + q * 11;
  const float o[3] = {row[0], row[1], row[2]}, d[3] = {row[3], row[4], row[5]};
  const float near = row[6], far = row[7];
  float n2 = near, f2 = far;
  const int r = rb_ray(c, o, d, near, far, &n2, &f2);
  if (bounds) {
    bounds[q * 2] = n2;
    bounds[q * 2 + 1] = f2;
  }
  if (hit) hit[q] = r != 0 ? 1 : 0;
  if (write_back && r == 2) {   // (otherwise the row already holds these two values)
    row[6] = n2;
    row[7] = f2;
  }
}

}  // namespace

extern "C" int fastnerf_occ_ray_bounds(const fn_occ_grid* grid, const fn_occ_cascade* cascade, int64_t n, float* rays11, int write_back,
                                       float* bounds, uint8_t* hit, fn_stream_t stream) {
  FN_CHECK_ARG((grid != nullptr) != (cascade != nullptr), "exactly one of grid / cascade");
  fn_occ_cascade one = {};
  if (grid) {
    one.levels = 1;
    one.level[0] = *grid;
    cascade = &one;
  }
  const char* fault = fn::occ_cascade_fault(cascade);
  FN_CHECK_ARG(!fault, fault ? fault : "");
  FN_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31), "0 <= n < 2^31");
  if (n == 0) return 0;
  FN_CHECK_ARG(rays11 && (write_back || bounds || hit), "non-null rays11, and write_back, bounds or hit to receive the result");
  RbDev c = {};
  int64_t cap = 16;
  for (int l = 0; l < cascade->levels; ++l) {
    const fn_occ_grid& g = cascade->level[l];
    for (int a = 0; a < 3; ++a) {
      c.g[l].lo[a] = g.lo[a];
      c.g[l].inv[a] = g.inv[a];
      c.g[l].n[a] = g.n[a];
      cap += 2 * (int64_t)g.n[a];
    }
    cap += 16;
    c.words[l] = g.words;
    c.outside = g.outside_occupied ? 1 : 0;   // of the LAST level
  }
  c.levels = cascade->levels;
  c.cap = (int)(cap < 0x7fffffff ? cap : 0x7fffffff);
  hipLaunchKernelGGL(ray_bounds_kernel, dim3((unsigned)((n + RB_BLOCK - 1) / RB_BLOCK)), dim3(RB_BLOCK), 0, fn::S(stream), c, n, rays11,
                     write_back, bounds, hit);
  FN_LAUNCH_CHECK();
  return 0;
}
