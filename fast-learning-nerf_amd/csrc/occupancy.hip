// occupancy.hip -- the occupancy grid of the inference path (include/fastnerf.h, "occupancy grid"): one bit per cell of a box
// [lo, hi) cut into nx x ny x nz cells, and the kernels that build it, look points up in it and sort the samples of a render
// pass by it, for gfx950.
//
// Bit layout (opaque to callers): cell (i, j, k) has the linear index c = (i * ny + j) * nz + k, bit c & 31 of word c >> 5.
// 256^3 cells are 2 MiB: the whole grid stays in an XCD's L2 while a pass is classified.
//
// The cell of a point x along one axis is floor((x - lo) * inv) with the subtraction and the product each rounded to fp32
// (fsub / fmul: no contraction), inv = n / (hi - lo) rounded once on the host.  An index outside 0 .. n-1 on any axis -- which
// is where every non-finite coordinate ends up, a NaN failing both comparisons -- takes the grid's `outside_occupied`.
//
// Kernels
//   occ_pack_kernel      cell predicate -> packed words, 64 cells per wave through one ballot.  Predicate: any of the cell's 8
//                        corner values of a point volume [nx+1, ny+1, nz+1] is > threshold (= their maximum is, for a volume
//                        without NaNs), or a byte mask [nx, ny, nz].
//   occ_dilate_kernel    OR over +-d cells along ONE axis; three launches (k, j, i) give the Chebyshev ball, clipped at the box
//   occ_query_kernel     [n, 3] points -> one byte each
//   occ_cell_points      training grid: one (jittered) point inside each cell of a cell range, as rays11 rows
//   occ_update_kernel    training grid: dens = max(dens * decay, relu(sigma)) on a cell range and, in the same launch, the
//                        bit dens > threshold of EVERY cell: one lane per cell, a wave's 64 consecutive cells are one ballot =
//                        two words, each stored by the one lane that owns it (no atomics)
//   occ_count / scatter  the samples o + d * z of a pass: per-block counts -> (the scan of train.hip) -> ascending list of the
//                        occupied sample indices; the others get raw = (0, 0, 0, 0).  The shape of fastnerf_compact_live with
//                        another predicate: deterministic, no atomics, the list length stays on the device.
//   The query / count / scatter kernels have ONE body each, instantiated for OccDev (one grid) and OccCascadeDev (a cascade of up
//   to 8 grids); the two occ_point overloads are all that differs.  In a cascade a point takes the bit of the FIRST level whose box
//   contains it, `outside` when none does.  The descriptors travel by value in the kernel argument (8 x 40 bytes of geometry, 8
//   pointers) and are read through scalar loads: the level loop's bounds and counter are wave-uniform, each lane leaves it at its
//   own level.  The six instantiations compile to the instructions of the kernels once written out per form (hipcc -S listings
//   compared with tools/isa_funcs.py: 11 kernels identical, 0 differ); timings: profiles/occupancy_render.md.
//   Early ray termination (fastnerf_ert_classify) is a further descriptor of the count / scatter kernels, ErtDev<G>: the entries of one
//   segment of B consecutive samples per ray, evaluated when the ray's transmittance is still > eps AND G (one grid, a cascade, or
//   OccAll = no grid) says occupied.  The instantiations above are untouched by it (isa_funcs.py: 11 identical, 0 differ).  The
//   transmittance itself is advanced by ert_advance_kernel in composite.hip, next to the compositing arithmetic it repeats.
//   The marched render (fastnerf_march_list) is one more, MarchDev: the entries of one segment of the packed rows of march.hip, evaluated
//   when the slot's lattice index is >= 0.  The lookup itself (descriptors, occ_point, the host checks) lives in occ_lookup.h, which
//   march.hip shares.
//   Training through a cascade (fastnerf_occ_cascade_own / _points / _update, at the end of the file): OwnDev is one more descriptor of the
//   count / scatter kernels -- entry q is cell q of a level, kept when no inner level covers it -- and the refresh kernels walk the
//   concatenation of the levels' own lists with the point and density arithmetic of the single grid (occ_cell_point, occ_dens_next).
// All of them are memory bound and small next to the MLP they spare: one lane per cell / point / four consecutive samples, a
// ray's 44 bytes come through the cache for all its samples.
#include "common.h"
#include "occ_lookup.h"   // OccDev, OccCascadeDev, occ_point, occ_dev / occ_cascade_dev: shared with march.hip

namespace fn {
void cp_scan_launch(int nb, int32_t* blk, int32_t* count_out, int n_points, hipStream_t st);   // train.hip
}

#define OCC_BLOCK 256
#define OCC_PTS 1024   // samples per block of the classify passes (256 threads x 4) = CP_PTS of train.hip, whose scan and
                       // fastnerf_compact_ws_ints this file reuses

namespace {

// early ray termination (fastnerf_ert_classify): no grid at all -- every point counts as occupied, and nothing of it is loaded
struct OccAll {};

// One segment [s0, s0 + w) of a pass's S samples per ray, sorted by the ray's transmittance and then by G (OccDev, OccCascadeDev
// or OccAll): entry q of the n * w samples of the segment is sample (q / w) * S + s0 + q % w of the pass, so ascending q is
// ascending sample index.  trans == NULL: every ray passes (the first segment, whose T is 1).
template <class G>
struct ErtDev {
  G g;
  const float* trans;
  float eps;
  uint32_t s0, w;
};

// The marched render (fastnerf_march_list, march.hip): one segment [s0, s0 + w) of the C slots of every packed row, sorted by the slot's
// lattice index alone -- kidx >= 0 is a live sample, -1 a closing entry or padding.  Entries as for ErtDev; no ray, no depth, no grid is read.
struct MarchDev {
  const int32_t* kidx;
  uint32_t s0, w;
};

// The own cells of one level of a training cascade (fastnerf_occ_cascade_own): entry q is cell q of the level, evaluated when no box
// of `box` holds it.  box[j] = (first, last) index per axis of the cells that inner level j covers -- worked out on the host in
// float64 from the levels' fp32 geometry, so the device compares integers only.  No ray, no depth, no bits are read.
struct OwnDev {
  int n[3];
  int nbox;
  int box[FN_OCC_MAX_LEVELS - 1][6];
};

__device__ __forceinline__ bool occ_point(const OccAll&, float, float, float) { return true; }

// the block's 256 predicate bits -> 8 words; every thread of the block calls it (c is the thread's cell, b false beyond the grid)
__device__ __forceinline__ void occ_store_bits(bool b, int64_t c, uint32_t* __restrict__ words, int64_t nwords) {
  const unsigned long long m = __ballot(b);
  const int lane = threadIdx.x & 63;
  const int64_t w = c >> 5;   // lanes 0 and 32 sit on word boundaries: a block starts at a multiple of 256 cells
  if (lane == 0 && w < nwords) words[w] = (uint32_t)m;
  if (lane == 32 && w < nwords) words[w] = (uint32_t)(m >> 32);
}

__device__ __forceinline__ void occ_ijk(int64_t c, const OccDims& d, int& i, int& j, int& k) {
  const uint32_t q = (uint32_t)c, r = q / (uint32_t)d.nz;   // ncells < 2^31
  k = (int)(q - r * (uint32_t)d.nz);
  i = (int)(r / (uint32_t)d.ny);
  j = (int)(r - (uint32_t)i * (uint32_t)d.ny);
}

template <bool FROM_MASK>
__global__ void __launch_bounds__(OCC_BLOCK) occ_pack_kernel(const float* __restrict__ vol, const uint8_t* __restrict__ mask, OccDims d,
                                                             float thr, uint32_t* __restrict__ words) {
  const int64_t c = (int64_t)blockIdx.x * OCC_BLOCK + threadIdx.x;
  bool b = false;
  if (c < d.ncells) {
    if (FROM_MASK) {
      b = mask[c] != 0;
    } else {
      int i, j, k;
      occ_ijk(c, d, i, j, k);
      const int64_t sy = d.nz + 1, sx = (int64_t)(d.ny + 1) * (d.nz + 1);
      const float* p = vol + i * sx + j * sy + k;
      b = (p[0] > thr) | (p[1] > thr) | (p[sy] > thr) | (p[sy + 1] > thr) | (p[sx] > thr) | (p[sx + 1] > thr) |
          (p[sx + sy] > thr) | (p[sx + sy + 1] > thr);
    }
  }
  occ_store_bits(b, c, words, d.nwords);
}

__global__ void __launch_bounds__(OCC_BLOCK) occ_dilate_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, OccDims d,
                                                               int axis, int r) {
  const int64_t c = (int64_t)blockIdx.x * OCC_BLOCK + threadIdx.x;
  bool b = false;
  if (c < d.ncells) {
    int ijk[3];
    occ_ijk(c, d, ijk[0], ijk[1], ijk[2]);
    const int len = axis == 0 ? d.nx : (axis == 1 ? d.ny : d.nz);
    const int64_t stride = axis == 0 ? (int64_t)d.ny * d.nz : (axis == 1 ? d.nz : 1);
    const int pos = ijk[axis];
    const int a = pos - r < 0 ? 0 : pos - r, e = pos + r > len - 1 ? len - 1 : pos + r;
    for (int q = a; q <= e && !b; ++q) b = occ_bit(src, (uint32_t)(c + (q - pos) * stride));
  }
  occ_store_bits(b, c, dst, d.nwords);
}

// G: OccDev or OccCascadeDev (occ_point picks the lookup)
template <class G>
__global__ void __launch_bounds__(OCC_BLOCK) occ_query_kernel(G g, int64_t n, const float* __restrict__ pts, uint8_t* __restrict__ out) {
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x)
    out[q] = occ_point(g, pts[q * 3], pts[q * 3 + 1], pts[q * 3 + 2]) ? 1 : 0;
}

__device__ __forceinline__ int occ_axis_cell(float x, float lo, float inv) { return (int)floorf(fmul(fsub(x, lo), inv)); }

// One point inside cell c of a grid with this geometry, as a rays11 row: x = lo + (index + jitter) / inv per axis, each operation rounded
// to fp32, jitter = 0.5 (jit == 0) or a Philox draw in [0, 1) keyed by (seed, cell).  Where fp32 rounding puts that point into a
// neighbouring cell (index + jitter rounds up to index + 1, or the sum lands on a face), the jitter is clamped towards the
// cell's centre -- halved distance to 0.5 per attempt, 0.5 itself at the end -- until occ_point's arithmetic gives the cell back.
// The one definition behind fastnerf_occ_cell_points and fastnerf_occ_cascade_points: a level's cell gets the bits its grid gives it.
__device__ __forceinline__ void occ_cell_point(const float* lo, const float* inv, const int* n, uint32_t c, uint32_t k0, uint32_t k1, int jit,
                                               float* __restrict__ row) {
  const uint32_t r = c / (uint32_t)n[2];
  int idx[3];
  idx[2] = (int)(c - r * (uint32_t)n[2]);
  idx[0] = (int)(r / (uint32_t)n[1]);
  idx[1] = (int)(r - (uint32_t)idx[0] * (uint32_t)n[1]);
  float u[3] = {0.5f, 0.5f, 0.5f};
  if (jit) {
    uint32_t o[4];
    philox4x32(c, 0u, 0x6f636367u, 0u, k0, k1, o);
    u[0] = u01(o[0]);
    u[1] = u01(o[1]);
    u[2] = u01(o[2]);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float j = u[a], x = 0.f;
    for (int it = 0; it < 26; ++it) {
      x = fadd(lo[a], __fdiv_rn(fadd((float)idx[a], j), inv[a]));
      if (occ_axis_cell(x, lo[a], inv[a]) == idx[a]) break;
      j = it < 24 ? fadd(0.5f, fmul(fsub(j, 0.5f), 0.5f)) : 0.5f;
    }
    row[a] = x;
  }
#pragma unroll
  for (int a = 3; a < 11; ++a) row[a] = 0.f;
}

// the cells c0 .. c0+n-1 of one grid
__global__ void __launch_bounds__(OCC_BLOCK) occ_cell_points_kernel(OccDev g, int64_t c0, int64_t n, uint32_t k0, uint32_t k1, int jit,
                                                                    float* __restrict__ rays11) {
  const int64_t q = (int64_t)blockIdx.x * OCC_BLOCK + threadIdx.x;
  if (q >= n) return;
  occ_cell_point(g.lo, g.inv, g.n, (uint32_t)(c0 + q), k0, k1, jit, rays11 + q * 11);
}

// dens' = max(dens * decay, relu(sigma_c), relu(sigma_f)) with the logits of row q; relu maps a NaN to 0
__device__ __forceinline__ float occ_dens_next(float v, const float* __restrict__ raw_c, const float* __restrict__ raw_f, int64_t q, float decay) {
  float s = raw_c[q * 4 + 3];
  s = s > 0.f ? s : 0.f;
  if (raw_f) {
    const float t = raw_f[q * 4 + 3];
    s = t > s ? t : s;
  }
  const float old = fmul(v, decay);
  return s > old ? s : old;
}

// sigma of cell c0 + q is raw_c[q * 4 + 3] (and raw_f's, the larger of the two counts); relu maps a NaN to 0.
__global__ void __launch_bounds__(OCC_BLOCK) occ_update_kernel(const float* __restrict__ raw_c, const float* __restrict__ raw_f, int64_t c0,
                                                               int64_t n, OccDims d, float decay, float thr, float* __restrict__ dens,
                                                               uint32_t* __restrict__ words) {
  const int64_t c = (int64_t)blockIdx.x * OCC_BLOCK + threadIdx.x;
  bool b = false;
  if (c < d.ncells) {
    float v = dens[c];
    const int64_t q = c - c0;
    if (q >= 0 && q < n) {
      v = occ_dens_next(v, raw_c, raw_f, q, decay);
      dens[c] = v;
    }
    b = v > thr;
  }
  if (words) occ_store_bits(b, c, words, d.nwords);   // (uniform: words == NULL updates the density only)
}

// entry q of a classify pass -> the sample index it stands for: itself, or the segment's sample (ErtDev)
template <class G>
__device__ __forceinline__ int64_t occ_sample(const G&, int64_t q, uint32_t) { return q; }
template <class G>
__device__ __forceinline__ int64_t occ_sample(const ErtDev<G>& e, int64_t q, uint32_t S) {
  const uint32_t r = (uint32_t)q / e.w;   // n * w <= n * S < 2^31
  return (int64_t)(r * S + e.s0 + ((uint32_t)q - r * e.w));
}
__device__ __forceinline__ int64_t occ_sample(const MarchDev& e, int64_t q, uint32_t S) {   // S = C, the slots of a row
  const uint32_t r = (uint32_t)q / e.w;
  return (int64_t)(r * S + e.s0 + ((uint32_t)q - r * e.w));
}

// sample p of the pass is evaluated: its point x = o + d * z (as the MLP kernels compute it) is occupied -- and, through an ErtDev,
// its ray's transmittance is still > eps (a NaN is not)
template <class G>
__device__ __forceinline__ bool occ_live(const G& g, const float* __restrict__ rays, const float* __restrict__ zv, uint32_t S, int64_t p) {
  const float* rr = rays + (int64_t)((uint32_t)p / S) * 11;   // n < 2^31
  const float zz = zv[p];
  return occ_point(g, fadd(rr[0], fmul(rr[3], zz)), fadd(rr[1], fmul(rr[4], zz)), fadd(rr[2], fmul(rr[5], zz)));
}
template <class G>
__device__ __forceinline__ bool occ_live(const ErtDev<G>& e, const float* __restrict__ rays, const float* __restrict__ zv, uint32_t S,
                                         int64_t p) {
  if (e.trans && !(e.trans[(uint32_t)p / S] > e.eps)) return false;
  return occ_live(e.g, rays, zv, S, p);
}
__device__ __forceinline__ bool occ_live(const MarchDev& e, const float* __restrict__, const float* __restrict__, uint32_t, int64_t p) {
  return e.kidx[p] >= 0;
}
// cell p of the level is its own: no inner level's box of covered cells holds it (e.nbox is uniform)
__device__ __forceinline__ bool occ_live(const OwnDev& e, const float* __restrict__, const float* __restrict__, uint32_t, int64_t p) {
  const uint32_t q = (uint32_t)p, r = q / (uint32_t)e.n[2];
  const int k = (int)(q - r * (uint32_t)e.n[2]), i = (int)(r / (uint32_t)e.n[1]), j = (int)(r - (uint32_t)i * (uint32_t)e.n[1]);
  bool covered = false;
  for (int b = 0; b < e.nbox; ++b)
    covered |= (i >= e.box[b][0]) & (i <= e.box[b][1]) & (j >= e.box[b][2]) & (j <= e.box[b][3]) & (k >= e.box[b][4]) & (k <= e.box[b][5]);
  return !covered;
}

// bits 0..3: entries p0 .. p0+3 of the pass are evaluated
template <class G>
__device__ __forceinline__ unsigned occ_flags(const G& g, const float* __restrict__ rays, const float* __restrict__ zv, uint32_t S,
                                              int64_t p0, int64_t n) {
  unsigned f = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (p0 + k < n && occ_live(g, rays, zv, S, occ_sample(g, p0 + k, S))) f |= 1u << k;
  }
  return f;
}

template <class G>
__global__ void __launch_bounds__(OCC_BLOCK) occ_count_kernel(G g, int64_t n, int S, const float* __restrict__ rays,
                                                              const float* __restrict__ zv, int* __restrict__ blk) {
  __shared__ int red[4];
  const unsigned f = occ_flags(g, rays, zv, (uint32_t)S, (int64_t)blockIdx.x * OCC_PTS + threadIdx.x * 4, n);
  int c = __popc(f);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) blk[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

template <class G>
__global__ void __launch_bounds__(OCC_BLOCK) occ_scatter_kernel(G g, int64_t n, int S, const float* __restrict__ rays,
                                                                const float* __restrict__ zv, const int* __restrict__ blk,
                                                                int* __restrict__ live_idx, float* __restrict__ raw) {
  __shared__ int wsum[4];
  const int64_t p0 = (int64_t)blockIdx.x * OCC_PTS + threadIdx.x * 4;
  const unsigned f = occ_flags(g, rays, zv, (uint32_t)S, p0, n);
  const int c = __popc(f);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int x = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(x, o, 64); if (lane >= o) x += t; }
  if (lane == 63) wsum[w] = x;
  __syncthreads();
  int pos = blk[blockIdx.x] + x - c;
  for (int k = 0; k < w; ++k) pos += wsum[k];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (f & (1u << k)) live_idx[pos++] = (int)occ_sample(g, p0 + k, (uint32_t)S);
    else if (raw && p0 + k < n) *reinterpret_cast<float4*>(raw + occ_sample(g, p0 + k, (uint32_t)S) * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// ---- host side (occ_dims, occ_geom, occ_dev, occ_cascade_dev: occ_lookup.h) ----------------------------------------
inline unsigned occ_blocks(int64_t ncells) { return (unsigned)((ncells + OCC_BLOCK - 1) / OCC_BLOCK); }

// the three dilation passes (k, j, i) of a grid whose undilated bits are in ws[0 .. nwords): -> words.  ws: 2 * nwords.
void occ_dilate_launch(const OccDims& d, int dilate, uint32_t* ws, uint32_t* words, hipStream_t s) {
  const dim3 g(occ_blocks(d.ncells)), b(OCC_BLOCK);
  uint32_t* a0 = ws;
  uint32_t* a1 = ws + d.nwords;
  hipLaunchKernelGGL(occ_dilate_kernel, g, b, 0, s, (const uint32_t*)a0, a1, d, 2, dilate);
  hipLaunchKernelGGL(occ_dilate_kernel, g, b, 0, s, (const uint32_t*)a1, a0, d, 1, dilate);
  hipLaunchKernelGGL(occ_dilate_kernel, g, b, 0, s, (const uint32_t*)a0, words, d, 0, dilate);
}

// the launches of fastnerf_occ_query / _cascade and fastnerf_occ_classify / _cascade (G: OccDev or OccCascadeDev); the callers
// keep the argument checks and FN_LAUNCH_CHECK, whose texts carry their own names
template <class G>
void occ_query_launch(const G& g, int64_t n, const float* pts, uint8_t* out, hipStream_t s) {
  const int64_t blocks = (n + OCC_BLOCK - 1) / OCC_BLOCK;
  hipLaunchKernelGGL(occ_query_kernel<G>, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(OCC_BLOCK), 0, s, g, n, pts, out);
}

// P: the entries of the pass (n * S samples, or the n * w of a segment)
template <class G>
void occ_classify_launch(const G& g, int64_t P, int S, const float* rays11, const float* z, int32_t* live_idx, int32_t* count_out,
                         float* raw, int32_t* ws, hipStream_t s) {
  const int nb = (int)((P + OCC_PTS - 1) / OCC_PTS);
  hipLaunchKernelGGL(occ_count_kernel<G>, dim3(nb), dim3(OCC_BLOCK), 0, s, g, P, S, rays11, z, ws);
  fn::cp_scan_launch(nb, ws, count_out, (int)P, s);
  hipLaunchKernelGGL(occ_scatter_kernel<G>, dim3(nb), dim3(OCC_BLOCK), 0, s, g, P, S, rays11, z, (const int*)ws, live_idx, raw);
}

}  // namespace

extern "C" int64_t fastnerf_occ_words(int64_t nx, int64_t ny, int64_t nz) {
  OccDims d;
  if (!occ_dims(nx, ny, nz, &d)) {
    fn::set_error("fastnerf_occ_words: bad argument: 1 <= nx, ny, nz <= 2^24 cells, fewer than 2^31 in all");
    return -1;
  }
  return d.nwords;
}

extern "C" int fastnerf_occ_build(const float* vol, int64_t nx, int64_t ny, int64_t nz, float threshold, int dilate, uint32_t* words,
                                  uint32_t* ws, fn_stream_t stream) {
  OccDims d;
  FN_CHECK_ARG(occ_dims(nx, ny, nz, &d), "1 <= nx, ny, nz <= 2^24 cells, fewer than 2^31 in all");
  FN_CHECK_ARG(vol && words && dilate >= 0 && (dilate == 0 || ws), "non-null vol / words, dilate >= 0, ws when dilate > 0");
  FN_CHECK_ARG(threshold == threshold, "threshold is a NaN");
  hipStream_t s = fn::S(stream);
  const dim3 g(occ_blocks(d.ncells)), b(OCC_BLOCK);
  hipLaunchKernelGGL(occ_pack_kernel<false>, g, b, 0, s, vol, (const uint8_t*)nullptr, d, threshold, dilate ? ws : words);
  if (dilate) occ_dilate_launch(d, dilate, ws, words, s);
  FN_LAUNCH_CHECK();
  return 0;
}

extern "C" int fastnerf_occ_from_mask(const uint8_t* mask, int64_t nx, int64_t ny, int64_t nz, uint32_t* words, fn_stream_t stream) {
  OccDims d;
  FN_CHECK_ARG(occ_dims(nx, ny, nz, &d), "1 <= nx, ny, nz <= 2^24 cells, fewer than 2^31 in all");
  FN_CHECK_ARG(mask && words, "non-null pointers");
  hipLaunchKernelGGL(occ_pack_kernel<true>, dim3(occ_blocks(d.ncells)), dim3(OCC_BLOCK), 0, fn::S(stream), (const float*)nullptr, mask, d,
                     0.f, words);
  FN_LAUNCH_CHECK();
  return 0;
}

extern "C" int fastnerf_occ_query(const fn_occ_grid* grid, int64_t n, const float* pts, uint8_t* out, fn_stream_t stream) {
  OccDev g;
  FN_CHECK_ARG(occ_dev(grid, &g), OCC_GRID_ARG);
  FN_CHECK_ARG(n >= 0, "n >= 0");
  if (n == 0) return 0;
  FN_CHECK_ARG(pts && out, "non-null pointers");
  occ_query_launch(g, n, pts, out, fn::S(stream));
  FN_LAUNCH_CHECK();
  return 0;
}

extern "C" int fastnerf_occ_cell_points(const fn_occ_grid* grid, int64_t c0, int64_t n, uint64_t seed, float* rays11, fn_stream_t stream) {
  OccDev g;
  FN_CHECK_ARG(occ_geom(grid, &g), "grid: 1 <= n[i] <= 2^24, fewer than 2^31 cells, finite lo, finite inv > 0 (the bits are not read)");
  const int64_t ncells = (int64_t)g.n[0] * g.n[1] * g.n[2];
  FN_CHECK_ARG(c0 >= 0 && n >= 0 && c0 <= ncells && n <= ncells - c0, "0 <= c0, c0 + n <= number of cells");
  if (n == 0) return 0;
  FN_CHECK_ARG(rays11, "non-null pointers");
  hipLaunchKernelGGL(occ_cell_points_kernel, dim3(occ_blocks(n)), dim3(OCC_BLOCK), 0, fn::S(stream), g, c0, n, (uint32_t)seed,
                     (uint32_t)(seed >> 32), seed != 0 ? 1 : 0, rays11);
  FN_LAUNCH_CHECK();
  return 0;
}

extern "C" int fastnerf_occ_update(const float* raw_c, const float* raw_f, int64_t c0, int64_t n, int64_t nx, int64_t ny, int64_t nz,
                                   float decay, float threshold, int dilate, float* dens, uint32_t* words, uint32_t* ws,
                                   fn_stream_t stream) {
  OccDims d;
  FN_CHECK_ARG(occ_dims(nx, ny, nz, &d), "1 <= nx, ny, nz <= 2^24 cells, fewer than 2^31 in all");
  FN_CHECK_ARG(c0 >= 0 && n >= 0 && c0 <= d.ncells && n <= d.ncells - c0, "0 <= c0, c0 + n <= number of cells");
  FN_CHECK_ARG(dens && (n == 0 || raw_c) && dilate >= 0 && (dilate == 0 || ws || !words),
               "non-null dens, raw_c when n > 0, dilate >= 0, ws when dilate > 0 and words are wanted");
  FN_CHECK_ARG(decay >= 0.f && decay <= 1.f && threshold == threshold, "0 <= decay <= 1, threshold is not a NaN");
  if (!words && n == 0) return 0;
  hipStream_t s = fn::S(stream);
  hipLaunchKernelGGL(occ_update_kernel, dim3(occ_blocks(d.ncells)), dim3(OCC_BLOCK), 0, s, raw_c, raw_f, c0, n, d, decay, threshold, dens,
                     !words ? (uint32_t*)nullptr : (dilate ? ws : words));
  if (words && dilate) occ_dilate_launch(d, dilate, ws, words, s);
  FN_LAUNCH_CHECK();
  return 0;
}

extern "C" int fastnerf_occ_classify(const fn_occ_grid* grid, int64_t n, int S, const float* rays11, const float* z, int32_t* live_idx,
                                     int32_t* count_out, float* raw, int32_t* ws, fn_stream_t stream) {
  OccDev g;
  FN_CHECK_ARG(occ_dev(grid, &g), OCC_GRID_ARG);
  FN_CHECK_ARG(n > 0 && S >= 1 && n * (int64_t)S < ((int64_t)1 << 31), "n > 0, S >= 1, n * S < 2^31");
  FN_CHECK_ARG(rays11 && z && live_idx && count_out && ws, "non-null pointers");
  occ_classify_launch(g, n * (int64_t)S, S, rays11, z, live_idx, count_out, raw, ws, fn::S(stream));
  FN_LAUNCH_CHECK();
  return 0;
}

// render.cpp checks a cascade (a grid: fastnerf_render_rays_fwd_ert) before it enqueues anything: NULL when every level is usable, else
// what is asked of one
namespace fn {
const char* occ_cascade_fault(const fn_occ_cascade* c) {
  OccCascadeDev d;
  return occ_cascade_dev(c, &d) ? nullptr : OCC_CASCADE_ARG;
}
const char* occ_grid_fault(const fn_occ_grid* g) {
  OccDev d;
  return occ_dev(g, &d) ? nullptr : OCC_GRID_ARG;
}
}  // namespace fn

extern "C" int fastnerf_occ_query_cascade(const fn_occ_cascade* cascade, int64_t n, const float* pts, uint8_t* out, fn_stream_t stream) {
  OccCascadeDev g;
  FN_CHECK_ARG(occ_cascade_dev(cascade, &g), OCC_CASCADE_ARG);
  FN_CHECK_ARG(n >= 0, "n >= 0");
  if (n == 0) return 0;
  FN_CHECK_ARG(pts && out, "non-null pointers");
  occ_query_launch(g, n, pts, out, fn::S(stream));
  FN_LAUNCH_CHECK();
  return 0;
}

extern "C" int fastnerf_occ_classify_cascade(const fn_occ_cascade* cascade, int64_t n, int S, const float* rays11, const float* z,
                                             int32_t* live_idx, int32_t* count_out, float* raw, int32_t* ws, fn_stream_t stream) {
  OccCascadeDev g;
  FN_CHECK_ARG(occ_cascade_dev(cascade, &g), OCC_CASCADE_ARG);
  FN_CHECK_ARG(n > 0 && S >= 1 && n * (int64_t)S < ((int64_t)1 << 31), "n > 0, S >= 1, n * S < 2^31");
  FN_CHECK_ARG(rays11 && z && live_idx && count_out && ws, "non-null pointers");
  occ_classify_launch(g, n * (int64_t)S, S, rays11, z, live_idx, count_out, raw, ws, fn::S(stream));
  FN_LAUNCH_CHECK();
  return 0;
}

// ---- early ray termination (include/fastnerf.h): one segment of the image pass sorted by T[ray] > eps AND the grid / cascade / nothing
template <class G>
static void ert_classify_launch(const G& g, int64_t n, int S, int s0, int s1, const float* rays11, const float* z, const float* trans,
                                float eps, int32_t* live_idx, int32_t* count_out, float* raw, int32_t* ws, hipStream_t s) {
  const ErtDev<G> e = {g, trans, eps, (uint32_t)s0, (uint32_t)(s1 - s0)};
  occ_classify_launch(e, n * (int64_t)(s1 - s0), S, rays11, z, live_idx, count_out, raw, ws, s);
}

extern "C" int fastnerf_ert_classify(const fn_occ_grid* grid, const fn_occ_cascade* cascade, int64_t n, int S, int s0, int s1,
                                     const float* rays11, const float* z, const float* trans, float eps, int32_t* live_idx,
                                     int32_t* count_out, float* raw, int32_t* ws, fn_stream_t stream) {
  OccDev g;
  OccCascadeDev c;
  FN_CHECK_ARG(!grid || !cascade, "at most one of grid / cascade");
  FN_CHECK_ARG(!grid || occ_dev(grid, &g), OCC_GRID_ARG);
  FN_CHECK_ARG(!cascade || occ_cascade_dev(cascade, &c), OCC_CASCADE_ARG);
  FN_CHECK_ARG(n > 0 && S >= 1 && n * (int64_t)S < ((int64_t)1 << 31), "n > 0, S >= 1, n * S < 2^31");
  FN_CHECK_ARG(s0 >= 0 && s0 < s1 && s1 <= S, "0 <= s0 < s1 <= S");
  FN_CHECK_ARG(eps >= 0.f && eps < 1.f, "0 <= eps < 1");
  FN_CHECK_ARG(rays11 && z && live_idx && count_out && ws, "non-null pointers");
  hipStream_t s = fn::S(stream);
  if (grid) ert_classify_launch(g, n, S, s0, s1, rays11, z, trans, eps, live_idx, count_out, raw, ws, s);
  else if (cascade) ert_classify_launch(c, n, S, s0, s1, rays11, z, trans, eps, live_idx, count_out, raw, ws, s);
  else ert_classify_launch(OccAll{}, n, S, s0, s1, rays11, z, trans, eps, live_idx, count_out, raw, ws, s);
  FN_LAUNCH_CHECK();
  return 0;
}

// ---- the marched render (include/fastnerf.h, "marched render"): the live list of one segment of the packed rows that fastnerf_occ_march wrote
// the render's counters: (evaluated so far, lattice points); one thread, behind the scan that wrote seg_count on the same stream
__global__ void march_total_kernel(const int32_t* __restrict__ seg_count, int first, int32_t lattice, int32_t* __restrict__ total) {
  total[0] = (first ? 0 : total[0]) + seg_count[0];
  total[1] = lattice;
}

extern "C" int fastnerf_march_list(int64_t n, int C, int s0, int s1, const int32_t* kidx, int32_t* live_idx, int32_t* count_out, float* raw,
                                   int32_t* ws, int32_t* total, int32_t lattice, fn_stream_t stream) {
  FN_CHECK_ARG(n > 0 && C >= 1 && n * (int64_t)C < ((int64_t)1 << 31), "n > 0, C >= 1, n * C < 2^31");
  FN_CHECK_ARG(s0 >= 0 && s0 < s1 && s1 <= C, "0 <= s0 < s1 <= C");
  FN_CHECK_ARG(kidx && live_idx && count_out && ws, "non-null pointers");
  const MarchDev m = {kidx, (uint32_t)s0, (uint32_t)(s1 - s0)};
  occ_classify_launch(m, n * (int64_t)(s1 - s0), C, (const float*)nullptr, (const float*)nullptr, live_idx, count_out, raw, ws, fn::S(stream));
  if (total) hipLaunchKernelGGL(march_total_kernel, dim3(1), dim3(1), 0, fn::S(stream), (const int32_t*)count_out, s0 == 0 ? 1 : 0, lattice, total);
  FN_LAUNCH_CHECK();
  return 0;
}

// ---- training through a cascade (include/fastnerf.h, "cascade, trained"): the own cells of a level, and the refresh over their concatenation
namespace {

#define OCC_TRAIN_ARG "cascade: 1 <= levels <= 8; every level: 1 <= n[i] <= 4096, finite lo, finite inv > 0"

// The concatenation of the levels' own lists, level 0 first: position p in [off[l], off[l+1]) is cell own[p] of level l.
struct OccSpan {
  const int32_t* own;
  int64_t off[FN_OCC_MAX_LEVELS + 1];
};

struct OccDensDev {
  float* dens[FN_OCC_MAX_LEVELS];
  float decay[FN_OCC_MAX_LEVELS];
  uint32_t ncells[FN_OCC_MAX_LEVELS];
};

// one rays11 row per position q0 .. q0+n-1: the point fastnerf_occ_cell_points makes for that level's grid and that cell.  l and
// g.levels are uniform (scalar loads of the level's geometry); a lane takes the level its position falls into.
__global__ void __launch_bounds__(OCC_BLOCK) occ_cascade_points_kernel(OccCascadeDev g, OccSpan s, int64_t q0, int64_t n, uint32_t k0, uint32_t k1,
                                                                       int jit, float* __restrict__ rays11) {
  const int64_t q = (int64_t)blockIdx.x * OCC_BLOCK + threadIdx.x;
  if (q >= n) return;
  const int64_t p = q0 + q;
  const uint32_t c = (uint32_t)s.own[p];
  for (int l = 0; l < g.levels; ++l)
    if (p >= s.off[l] && p < s.off[l + 1]) occ_cell_point(g.g[l].lo, g.g[l].inv, g.g[l].n, c, k0, k1, jit, rays11 + q * 11);
}

// dens = max(dens * decay, relu(sigma_c), relu(sigma_f)) of the cell of each position: every cell stands once in the concatenation, so
// every store has one writer.  (c < ncells holds for a list made by fastnerf_occ_cascade_own; a foreign list cannot write outside dens)
__global__ void __launch_bounds__(OCC_BLOCK) occ_cascade_update_kernel(OccDensDev d, OccSpan s, int levels, const float* __restrict__ raw_c,
                                                                       const float* __restrict__ raw_f, int64_t q0, int64_t n) {
  const int64_t q = (int64_t)blockIdx.x * OCC_BLOCK + threadIdx.x;
  if (q >= n) return;
  const int64_t p = q0 + q;
  const uint32_t c = (uint32_t)s.own[p];
  for (int l = 0; l < levels; ++l)
    if (p >= s.off[l] && p < s.off[l + 1] && c < d.ncells[l]) d.dens[l][c] = occ_dens_next(d.dens[l][c], raw_c, raw_f, q, d.decay[l]);
}

// the geometry of a training cascade (the bits are not read: words may be NULL)
bool occ_train_dev(const fn_occ_cascade* c, OccCascadeDev* o) {
  if (!c || c->levels < 1 || c->levels > FN_OCC_MAX_LEVELS) return false;
  *o = OccCascadeDev{};
  for (int l = 0; l < c->levels; ++l) {
    OccDev d;
    if (!occ_geom(&c->level[l], &d)) return false;
    for (int a = 0; a < 3; ++a) {
      if (d.n[a] > 4096) return false;
      o->g[l].lo[a] = d.lo[a];
      o->g[l].inv[a] = d.inv[a];
      o->g[l].n[a] = d.n[a];
    }
    o->words[l] = d.words;
  }
  o->levels = c->levels;
  return true;
}

// offsets[levels + 1] (host): 0 = offsets[0] <= offsets[1] <= ..., no level longer than its grid, and [q0, q0 + n) inside
bool occ_span(const OccCascadeDev& g, const int32_t* own, const int64_t* offsets, int64_t q0, int64_t n, OccSpan* s) {
  if (!offsets || offsets[0] != 0 || q0 < 0 || n < 0) return false;
  *s = OccSpan{};
  s->own = own;
  for (int l = 0; l < g.levels; ++l) {
    const int64_t len = offsets[l + 1] - offsets[l];
    if (len < 0 || len > (int64_t)g.g[l].n[0] * g.g[l].n[1] * g.g[l].n[2]) return false;
    s->off[l + 1] = offsets[l + 1];
  }
  return q0 <= offsets[g.levels] && n <= offsets[g.levels] - q0;
}

}  // namespace

extern "C" int fastnerf_occ_cascade_own(const fn_occ_cascade* cascade, int level, int dilate, int32_t* list, int32_t* count_out, int32_t* ws,
                                        fn_stream_t stream) {
  OccCascadeDev g;
  FN_CHECK_ARG(occ_train_dev(cascade, &g), OCC_TRAIN_ARG);
  FN_CHECK_ARG(level >= 0 && level < g.levels && dilate >= 0 && dilate <= 4096, "0 <= level < levels, 0 <= dilate <= 4096");
  FN_CHECK_ARG(list && count_out && ws, "non-null pointers");
  // Per inner level j and axis a, in float64 with every product and sum rounded on its own (this file is compiled without
  // contraction): w = 1 / inv, hi = lo + n w; cell i of `level` is covered on the axis when
  //   lo_l + (i - m) w_l >= lo_j + w_j   and   lo_l + (i + 1 + m) w_l <= hi_j - w_j,   m = dilate + 1.
  // Both sides are monotone in i, so the covered indices of an axis are one interval [first, last].
  const OccLevel& L = g.g[level];
  OwnDev e = {};
  const int m = dilate + 1;
  for (int a = 0; a < 3; ++a) e.n[a] = L.n[a];
  for (int j = 0; j < level; ++j) {
    const OccLevel& J = g.g[j];
    int* box = e.box[e.nbox];
    bool any = true;
    for (int a = 0; a < 3 && any; ++a) {
      const double wl = 1.0 / (double)L.inv[a], wj = 1.0 / (double)J.inv[a];
      const double lol = (double)L.lo[a], loj = (double)J.lo[a];
      const double hij = loj + (double)J.n[a] * wj;
      const double A = loj + wj, B = hij - wj;
      int first = L.n[a], last = -1;
      for (int i = 0; i < L.n[a]; ++i) {
        const double left = lol + (double)(i - m) * wl, right = lol + (double)(i + 1 + m) * wl;
        if (left >= A && right <= B) {
          if (i < first) first = i;
          last = i;
        }
      }
      box[2 * a] = first;
      box[2 * a + 1] = last;
      any = last >= first;
    }
    if (any) ++e.nbox;
  }
  occ_classify_launch(e, (int64_t)L.n[0] * L.n[1] * L.n[2], 1, (const float*)nullptr, (const float*)nullptr, list, count_out, (float*)nullptr, ws,
                      fn::S(stream));
  FN_LAUNCH_CHECK();
  return 0;
}

extern "C" int fastnerf_occ_cascade_points(const fn_occ_cascade* cascade, const int32_t* own, const int64_t* offsets, int64_t q0, int64_t n,
                                           uint64_t seed, float* rays11, fn_stream_t stream) {
  OccCascadeDev g;
  OccSpan s;
  FN_CHECK_ARG(occ_train_dev(cascade, &g), OCC_TRAIN_ARG);
  FN_CHECK_ARG(occ_span(g, own, offsets, q0, n, &s), "offsets[0] = 0, ascending, no level longer than its grid; 0 <= q0, q0 + n <= offsets[levels]");
  if (n == 0) return 0;
  FN_CHECK_ARG(own && rays11, "non-null pointers");
  hipLaunchKernelGGL(occ_cascade_points_kernel, dim3(occ_blocks(n)), dim3(OCC_BLOCK), 0, fn::S(stream), g, s, q0, n, (uint32_t)seed,
                     (uint32_t)(seed >> 32), seed != 0 ? 1 : 0, rays11);
  FN_LAUNCH_CHECK();
  return 0;
}

extern "C" int fastnerf_occ_cascade_update(const fn_occ_cascade* cascade, const float* raw_c, const float* raw_f, const int32_t* own,
                                           const int64_t* offsets, int64_t q0, int64_t n, const float* decay, float* const* dens,
                                           fn_stream_t stream) {
  OccCascadeDev g;
  OccSpan s;
  FN_CHECK_ARG(occ_train_dev(cascade, &g), OCC_TRAIN_ARG);
  FN_CHECK_ARG(occ_span(g, own, offsets, q0, n, &s), "offsets[0] = 0, ascending, no level longer than its grid; 0 <= q0, q0 + n <= offsets[levels]");
  FN_CHECK_ARG(decay && dens, "non-null decay / dens");
  OccDensDev d = {};
  for (int l = 0; l < g.levels; ++l) {
    FN_CHECK_ARG(dens[l] && decay[l] >= 0.f && decay[l] <= 1.f, "every level: non-null dens, 0 <= decay <= 1");
    d.dens[l] = dens[l];
    d.decay[l] = decay[l];
    d.ncells[l] = (uint32_t)((int64_t)g.g[l].n[0] * g.g[l].n[1] * g.g[l].n[2]);
  }
  if (n == 0) return 0;
  FN_CHECK_ARG(own && raw_c, "non-null pointers");
  hipLaunchKernelGGL(occ_cascade_update_kernel, dim3(occ_blocks(n)), dim3(OCC_BLOCK), 0, fn::S(stream), d, s, g.levels, raw_c, raw_f, q0, n);
  FN_LAUNCH_CHECK();
  return 0;
}
