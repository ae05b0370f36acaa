// mesh.hip -- mesh extraction (nerf-ours/extract_mesh.py:38-74): the points of the dense density query and marching
// cubes over the resulting volume, for gfx950.
//
// Marching cubes over a float32 volume [nx, ny, nz] (C order, k fastest); inside = value > thr.  The output contract
// (include/fastnerf.h) is deterministic: one vertex per crossing grid edge, ordered by the lower endpoint's linear
// index and then by axis i, j, k; triangles ordered by cell and then in table order (csrc/mc_tables.h).  A cell is
// named by its lower corner point, so point order is cell order and every pass runs over points, MC_BLOCK per block:
//   1. mc_count_kernel  per block: (vertices, triangles)                                -> level 0
//   2. mc_scan_kernel   exclusive scan of level L in groups of MC_BLOCK, group totals  -> level L+1, until one group
//                       is left (level K = the totals).  A block's offset is the sum of its entries over the levels, so
//                       there is no down-sweep launch.
//   3. mc_vert_kernel   vertices, plus the per-point vertex base and crossing mask
//   4. mc_tri_kernel    triangles: the cell's edges become vertex indices through those bases
// No atomics anywhere: two runs are bit-identical.  Memory-bound; the volume is read three times (each pass reads a
// point's up-to-8 corners, mostly from L2) and the base / mask arrays (5 B per point) are written once and read once.
#include "common.h"
#include "mc_tables.h"

#define MC_BLOCK 256        // points per block in every pass; elements per scan group
#define MC_MAX_LEVELS 8     // scan levels: 256^8 blocks is beyond any volume that fits in memory

__constant__ int8_t c_mc_tri[256][MC_TRI_STRIDE] = MC_TRI_TABLE_INIT;
__constant__ uint8_t c_mc_ntri[256] = MC_NTRI_INIT;
__constant__ int8_t c_mc_corner[8][3] = MC_CORNER_INIT;
__constant__ int8_t c_mc_edge_lo[12] = MC_EDGE_LO_INIT;
__constant__ int8_t c_mc_edge_axis[12] = MC_EDGE_AXIS_INIT;
static const int8_t h_mc_tri[256][MC_TRI_STRIDE] = MC_TRI_TABLE_INIT;
static const uint16_t h_mc_edge[256] = MC_EDGE_TABLE_INIT;

namespace {

struct McDims {
  int64_t nx, ny, nz, npts, nb;   // nb: blocks of MC_BLOCK points
  float thr;
};

struct McLevels {
  longlong2* lv[MC_MAX_LEVELS + 1];   // lv[0..K-1]: exclusive scans; lv[K][0]: (vertices, triangles) in all
  int K;
};

__device__ __forceinline__ int64_t mc_block_id() { return (int64_t)blockIdx.y * gridDim.x + blockIdx.x; }

__device__ __forceinline__ void mc_ijk(int64_t p, const McDims& d, int64_t& i, int64_t& j, int64_t& k) {
  if (d.npts <= 0xffffffffLL) {   // 32-bit division where the index fits
    const uint32_t q = (uint32_t)p, nz = (uint32_t)d.nz, ny = (uint32_t)d.ny;
    const uint32_t r = q / nz;
    k = q - r * nz;
    i = r / ny;
    j = r - (uint32_t)i * ny;
  } else {
    const int64_t r = p / d.nz;
    k = p - r * d.nz;
    i = r / d.ny;
    j = r - i * d.ny;
  }
}

// crossing mask of point p's +i / +j / +k edges (bits 0..2) and, when p is a cell's lower corner, the cell's case
struct McPoint {
  unsigned mask, cas;
  bool cell;
};
__device__ __forceinline__ McPoint mc_classify(const float* __restrict__ vol, int64_t p, const McDims& d) {
  int64_t i, j, k;
  mc_ijk(p, d, i, j, k);
  const int64_t sy = d.nz, sx = d.ny * d.nz;
  const bool hi = i + 1 < d.nx, hj = j + 1 < d.ny, hk = k + 1 < d.nz;
  McPoint r;
  r.cell = hi && hj && hk;
  r.cas = 0;
  if (r.cell) {
#pragma unroll
    for (int n = 0; n < 8; ++n) {
      const int64_t q = p + c_mc_corner[n][0] * sx + c_mc_corner[n][1] * sy + c_mc_corner[n][2];
      r.cas |= (unsigned)(vol[q] > d.thr) << n;
    }
    const unsigned in0 = r.cas & 1u;   // corners 1, 3, 4 are p + e_i, p + e_j, p + e_k
    r.mask = (((r.cas >> 1) & 1u) ^ in0) | ((((r.cas >> 3) & 1u) ^ in0) << 1) | ((((r.cas >> 4) & 1u) ^ in0) << 2);
  } else {
    const bool in0 = vol[p] > d.thr;
    r.mask = (unsigned)(hi && ((vol[p + sx] > d.thr) != in0)) | ((unsigned)(hj && ((vol[p + sy] > d.thr) != in0)) << 1) |
             ((unsigned)(hk && ((vol[p + 1] > d.thr) != in0)) << 2);
  }
  return r;
}

// exclusive prefix of x over the block's MC_BLOCK threads (thread order); *total = the block's sum.  Every thread calls it.
template <typename T>
__device__ __forceinline__ T mc_block_scan(T x, T* total) {
  __shared__ T wsum[MC_BLOCK / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  T incl = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  T pre = 0, all = 0;
#pragma unroll
  for (int q = 0; q < MC_BLOCK / 64; ++q) {
    pre += (q < w) ? wsum[q] : (T)0;
    all += wsum[q];
  }
  *total = all;
  return pre + incl - x;
}

__device__ __forceinline__ longlong2 mc_offset(const McLevels& L, int64_t b) {
  long long x = 0, y = 0;
  for (int l = 0; l < L.K; ++l) {
    const longlong2 v = L.lv[l][b];
    x += v.x;
    y += v.y;
    b /= MC_BLOCK;
  }
  return make_longlong2(x, y);
}

__global__ void __launch_bounds__(MC_BLOCK) mc_count_kernel(const float* __restrict__ vol, McDims d, longlong2* __restrict__ lv0) {
  const int64_t b = mc_block_id();
  if (b >= d.nb) return;   // whole block
  const int64_t p = b * MC_BLOCK + threadIdx.x;
  int packed = 0;          // vertices (<= 3) | triangles (<= 5) << 16; a block's sums stay below 2^16 each
  if (p < d.npts) {
    const McPoint pt = mc_classify(vol, p, d);
    packed = __popc(pt.mask) | ((pt.cell ? (int)c_mc_ntri[pt.cas] : 0) << 16);
  }
  int total;
  mc_block_scan(packed, &total);
  if (threadIdx.x == 0) lv0[b] = make_longlong2(total & 0xffff, total >> 16);
}

__global__ void __launch_bounds__(MC_BLOCK) mc_scan_kernel(int64_t n, longlong2* __restrict__ a, longlong2* __restrict__ up) {
  const int64_t g = mc_block_id();
  if (g * MC_BLOCK >= n) return;
  const int64_t i = g * MC_BLOCK + threadIdx.x;
  const longlong2 v = (i < n) ? a[i] : make_longlong2(0, 0);
  long long tx, ty;
  const long long ex = mc_block_scan((long long)v.x, &tx);
  __syncthreads();   // mc_block_scan<long long> reuses its LDS
  const long long ey = mc_block_scan((long long)v.y, &ty);
  if (i < n) a[i] = make_longlong2(ex, ey);
  if (threadIdx.x == 0) up[g] = make_longlong2(tx, ty);
}

__global__ void __launch_bounds__(MC_BLOCK) mc_vert_kernel(const float* __restrict__ vol, McDims d, McLevels L,
                                                            int32_t* __restrict__ vbase, uint8_t* __restrict__ pmask,
                                                            float* __restrict__ verts) {
  const int64_t b = mc_block_id();
  if (b >= d.nb) return;
  const int64_t p = b * MC_BLOCK + threadIdx.x;
  McPoint pt = {0u, 0u, false};
  if (p < d.npts) pt = mc_classify(vol, p, d);
  int total;
  const int loc = mc_block_scan((int)__popc(pt.mask), &total);
  if (p >= d.npts) return;
  const int64_t vb = mc_offset(L, b).x + loc;
  vbase[p] = (int32_t)vb;   // < 2^31: fastnerf_mc_count refused anything larger
  pmask[p] = (uint8_t)pt.mask;
  if (!pt.mask) return;
  int64_t i, j, k;
  mc_ijk(p, d, i, j, k);
  const int64_t stride[3] = {d.ny * d.nz, d.nz, 1};
  const float v0 = vol[p];
  int64_t o = vb * 3;
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    if (!((pt.mask >> ax) & 1u)) continue;
    const float v1 = vol[p + stride[ax]];
    const float t = __fdiv_rn(fsub(d.thr, v0), fsub(v1, v0));
    float c[3] = {(float)i, (float)j, (float)k};
    c[ax] = fadd(c[ax], t);
    verts[o + 0] = c[0];
    verts[o + 1] = c[1];
    verts[o + 2] = c[2];
    o += 3;
  }
}

__global__ void __launch_bounds__(MC_BLOCK) mc_tri_kernel(const float* __restrict__ vol, McDims d, McLevels L,
                                                           const int32_t* __restrict__ vbase, const uint8_t* __restrict__ pmask,
                                                           int32_t* __restrict__ tris) {
  const int64_t b = mc_block_id();
  if (b >= d.nb) return;
  const int64_t p = b * MC_BLOCK + threadIdx.x;
  McPoint pt = {0u, 0u, false};
  if (p < d.npts) pt = mc_classify(vol, p, d);
  const int nt = pt.cell ? (int)c_mc_ntri[pt.cas] : 0;
  int total;
  const int loc = mc_block_scan(nt, &total);
  if (nt == 0) return;
  int64_t o = (mc_offset(L, b).y + loc) * 3;
  const int64_t sy = d.nz, sx = d.ny * d.nz;
  for (int e3 = 0; e3 < 3 * nt; ++e3) {
    const int e = c_mc_tri[pt.cas][e3];
    const int c = c_mc_edge_lo[e], ax = c_mc_edge_axis[e];
    const int64_t q = p + c_mc_corner[c][0] * sx + c_mc_corner[c][1] * sy + c_mc_corner[c][2];
    tris[o + e3] = vbase[q] + __popc((unsigned)pmask[q] & ((1u << ax) - 1u));
  }
}

// ---- grid query: the chunk [p0, p0 + n) of the points (xs[i], ys[j], zs[k]) as rays11 rows o = point, d = 0, near = far = 0,
// viewdir = 0 -- exactly what run_nerf.run_network builds for explicit points -- and relu(sigma) of the MLP's output rows
__global__ void __launch_bounds__(256) grid_points_kernel(int64_t p0, int64_t n, const float* __restrict__ xs, int64_t ny,
                                                          const float* __restrict__ ys, int64_t nz, const float* __restrict__ zs,
                                                          float* __restrict__ rays11) {
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = p0 + q;
    const int64_t r = p / nz, k = p - r * nz, i = r / ny, j = r - i * ny;
    float* row = rays11 + q * 11;
    row[0] = xs[i];
    row[1] = ys[j];
    row[2] = zs[k];
#pragma unroll
    for (int c = 3; c < 11; ++c) row[c] = 0.f;
  }
}

__global__ void __launch_bounds__(256) grid_sigma_kernel(int64_t n, const float* __restrict__ raw, float* __restrict__ out) {
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
    const float s = raw[q * 4 + 3];
    out[q] = (s < 0.f) ? 0.f : s;   // relu; a NaN stays a NaN, as in torch.relu / np.maximum
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------
constexpr int64_t kAlign = 256;
inline int64_t align_up(int64_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

// workspace layout: vbase int32[npts] | pmask uint8[npts] | scan levels (longlong2) 0..K.  Returns bytes, or -1.
int64_t mc_plan(int64_t nx, int64_t ny, int64_t nz, McDims* d, int64_t off[MC_MAX_LEVELS + 1], int* K) {
  if (nx < 2 || ny < 2 || nz < 2) return -1;
  if (nx > ((int64_t)1 << 40) / ny / nz) return -1;   // > 2^40 points: far beyond device memory
  d->nx = nx;
  d->ny = ny;
  d->nz = nz;
  d->npts = nx * ny * nz;
  d->nb = (d->npts + MC_BLOCK - 1) / MC_BLOCK;
  int64_t cur = align_up(align_up(d->npts * 4) + d->npts);
  int64_t n = d->nb;
  int l = 0;
  for (;;) {
    off[l] = cur;
    cur = align_up(cur + n * (int64_t)sizeof(longlong2));
    if (l > 0 && n == 1) break;
    n = (n + MC_BLOCK - 1) / MC_BLOCK;
    ++l;
  }
  *K = l;
  return cur;
}

dim3 mc_grid(int64_t nb) {
  const int64_t gx = nb < ((int64_t)1 << 20) ? nb : ((int64_t)1 << 20);
  return dim3((unsigned)gx, (unsigned)((nb + gx - 1) / gx));
}

McLevels mc_levels(void* ws, const int64_t off[], int K) {
  McLevels L;
  for (int l = 0; l <= MC_MAX_LEVELS; ++l) L.lv[l] = l <= K ? reinterpret_cast<longlong2*>((char*)ws + off[l]) : nullptr;
  L.K = K;
  return L;
}

}  // namespace

extern "C" int64_t fastnerf_mc_ws_bytes(int64_t nx, int64_t ny, int64_t nz) {
  McDims d;
  int64_t off[MC_MAX_LEVELS + 1];
  int K;
  const int64_t bytes = mc_plan(nx, ny, nz, &d, off, &K);
  if (bytes < 0) fn::set_error("fastnerf_mc_ws_bytes: bad argument: every dimension >= 2, at most 2^40 points");
  return bytes;
}

extern "C" int fastnerf_mc_count(const float* vol, int64_t nx, int64_t ny, int64_t nz, float thr, void* ws, int64_t* counts_host,
                                 fn_stream_t stream) {
  McDims d;
  int64_t off[MC_MAX_LEVELS + 1];
  int K;
  FN_CHECK_ARG(mc_plan(nx, ny, nz, &d, off, &K) >= 0, "every dimension >= 2, at most 2^40 points");
  FN_CHECK_ARG(vol && ws && counts_host, "non-null pointers");
  d.thr = thr;
  const McLevels L = mc_levels(ws, off, K);
  hipStream_t s = fn::S(stream);
  hipLaunchKernelGGL(mc_count_kernel, mc_grid(d.nb), dim3(MC_BLOCK), 0, s, vol, d, L.lv[0]);
  int64_t n = d.nb;
  for (int l = 0; l < K; ++l) {
    const int64_t groups = (n + MC_BLOCK - 1) / MC_BLOCK;
    hipLaunchKernelGGL(mc_scan_kernel, mc_grid(groups), dim3(MC_BLOCK), 0, s, n, L.lv[l], L.lv[l + 1]);
    n = groups;
  }
  FN_LAUNCH_CHECK();
  longlong2 tot;
  FN_HIP(hipMemcpyAsync(&tot, L.lv[K], sizeof(tot), hipMemcpyDeviceToHost, s));
  FN_HIP(hipStreamSynchronize(s));
  counts_host[0] = tot.x;
  counts_host[1] = tot.y;
  if (tot.x > INT32_MAX || tot.y > INT32_MAX) {
    fn::set_error("fastnerf_mc_count: %lld vertices / %lld triangles: more than 2^31-1", (long long)tot.x, (long long)tot.y);
    return -1;
  }
  return 0;
}

extern "C" int fastnerf_mc_emit(const float* vol, int64_t nx, int64_t ny, int64_t nz, float thr, void* ws, float* verts,
                                int32_t* tris, fn_stream_t stream) {
  McDims d;
  int64_t off[MC_MAX_LEVELS + 1];
  int K;
  FN_CHECK_ARG(mc_plan(nx, ny, nz, &d, off, &K) >= 0, "every dimension >= 2, at most 2^40 points");
  FN_CHECK_ARG(vol && ws && verts && tris, "non-null pointers");
  d.thr = thr;
  const McLevels L = mc_levels(ws, off, K);
  int32_t* vbase = reinterpret_cast<int32_t*>(ws);
  uint8_t* pmask = reinterpret_cast<uint8_t*>((char*)ws + align_up(d.npts * 4));
  hipStream_t s = fn::S(stream);
  hipLaunchKernelGGL(mc_vert_kernel, mc_grid(d.nb), dim3(MC_BLOCK), 0, s, vol, d, L, vbase, pmask, verts);
  hipLaunchKernelGGL(mc_tri_kernel, mc_grid(d.nb), dim3(MC_BLOCK), 0, s, vol, d, L, vbase, pmask, tris);
  FN_LAUNCH_CHECK();
  return 0;
}

extern "C" int fastnerf_mc_tables(int8_t* tri_host, uint16_t* edge_host) {
  FN_CHECK_ARG(tri_host && edge_host, "non-null pointers");
  for (int c = 0; c < 256; ++c) {
    for (int e = 0; e < MC_TRI_STRIDE; ++e) tri_host[c * MC_TRI_STRIDE + e] = h_mc_tri[c][e];
    edge_host[c] = h_mc_edge[c];
  }
  return 0;
}

extern "C" int fastnerf_grid_points(int64_t p0, int64_t n, const float* xs, int64_t nx, const float* ys, int64_t ny,
                                    const float* zs, int64_t nz, float* rays11, fn_stream_t stream) {
  FN_CHECK_ARG(nx > 0 && ny > 0 && nz > 0 && p0 >= 0 && n >= 0 && nx <= INT64_MAX / ny / nz && p0 + n <= nx * ny * nz,
               "0 <= p0, p0 + n <= nx*ny*nz");
  if (n == 0) return 0;
  FN_CHECK_ARG(xs && ys && zs && rays11, "non-null pointers");
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(grid_points_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, fn::S(stream), p0, n, xs,
                     ny, ys, nz, zs, rays11);
  FN_LAUNCH_CHECK();
  return 0;
}

extern "C" int fastnerf_grid_sigma(int64_t n, const float* raw, float* out, fn_stream_t stream) {
  FN_CHECK_ARG(n >= 0, "n >= 0");
  if (n == 0) return 0;
  FN_CHECK_ARG(raw && out, "non-null pointers");
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(grid_sigma_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, fn::S(stream), n, raw, out);
  FN_LAUNCH_CHECK();
  return 0;
}
