// occ_lookup.h -- the lookup of the occupancy grid (include/fastnerf.h, "occupancy grid"): the device descriptors of one grid and of a
// cascade, occ_point, and the host checks that fill a descriptor from the caller's struct.  Included by occupancy.hip (build, query,
// classify) and march.hip (the marched render): one definition of the index arithmetic, hence one set of bits.  Everything has internal
// linkage; the kernels that take a descriptor are instantiated in the translation unit that launches them.
#pragma once
#include "common.h"

#define OCC_GRID_ARG "grid: non-null words, 1 <= n[i] <= 2^24, fewer than 2^31 cells, finite lo, finite inv > 0"
#define OCC_CASCADE_ARG "cascade: 1 <= levels <= 8; every level: non-null words, 1 <= n[i] <= 2^24, fewer than 2^31 cells, finite lo, finite inv > 0"

namespace {

struct OccDev {
  const uint32_t* words;
  float lo[3], inv[3];
  int n[3];
  int outside;
};

// a cascade (fn_occ_cascade): per level the geometry of OccDev (40 bytes) and, apart from it, the pointer to its bits
struct OccLevel {
  float lo[3], inv[3];
  int n[3];
  int pad;
};

struct OccCascadeDev {
  OccLevel g[FN_OCC_MAX_LEVELS];
  const uint32_t* words[FN_OCC_MAX_LEVELS];
  int levels;
  int outside;
};

struct OccDims {
  int nx, ny, nz;
  int64_t ncells, nwords;
};

__device__ __forceinline__ bool occ_bit(const uint32_t* __restrict__ words, uint32_t c) { return (words[c >> 5] >> (c & 31u)) & 1u; }

// The lookup in two steps, so that a caller with several independent points can issue their loads together (march.hip): occ_locate does
// the index arithmetic -- true: the point takes bit `cell` of `words`; false: it takes `outside`, and (words, cell) name bit 0 of the
// first grid, which exists, so a load issued regardless stays in bounds -- and occ_point is occ_locate + the one load.
__device__ __forceinline__ bool occ_locate(const OccDev& g, float x, float y, float z, const uint32_t*& words, uint32_t& cell) {
  const float fi = floorf(fmul(fsub(x, g.lo[0]), g.inv[0]));
  const float fj = floorf(fmul(fsub(y, g.lo[1]), g.inv[1]));
  const float fk = floorf(fmul(fsub(z, g.lo[2]), g.inv[2]));
  const bool inside = fi >= 0.f && fi < (float)g.n[0] && fj >= 0.f && fj < (float)g.n[1] && fk >= 0.f && fk < (float)g.n[2];
  words = g.words;
  cell = inside ? ((uint32_t)fi * (uint32_t)g.n[1] + (uint32_t)fj) * (uint32_t)g.n[2] + (uint32_t)fk : 0u;
  return inside;
}

// one level of a cascade: the level's box contains the point, whose cell is then `cell`
__device__ __forceinline__ bool occ_level(const OccLevel& g, float x, float y, float z, uint32_t& cell) {
  const float fi = floorf(fmul(fsub(x, g.lo[0]), g.inv[0]));
  const float fj = floorf(fmul(fsub(y, g.lo[1]), g.inv[1]));
  const float fk = floorf(fmul(fsub(z, g.lo[2]), g.inv[2]));
  cell = ((uint32_t)fi * (uint32_t)g.n[1] + (uint32_t)fj) * (uint32_t)g.n[2] + (uint32_t)fk;
  // (& not &&: one straight-line test per level, its 40 bytes of geometry fetched by one batch of scalar loads)
  return (fi >= 0.f) & (fi < (float)g.n[0]) & (fj >= 0.f) & (fj < (float)g.n[1]) & (fk >= 0.f) & (fk < (float)g.n[2]);
}

// first level whose box contains the point decides; l and c.levels are uniform, so g[l] and words[l] are scalar loads
__device__ __forceinline__ bool occ_locate(const OccCascadeDev& c, float x, float y, float z, const uint32_t*& words, uint32_t& cell) {
  for (int l = 0; l < c.levels; ++l) {
    if (occ_level(c.g[l], x, y, z, cell)) {
      words = c.words[l];
      return true;
    }
  }
  words = c.words[0];
  cell = 0u;
  return false;
}

__device__ __forceinline__ int occ_outside(const OccDev& g) { return g.outside; }
__device__ __forceinline__ int occ_outside(const OccCascadeDev& c) { return c.outside; }

__device__ __forceinline__ bool occ_point(const OccDev& g, float x, float y, float z) {
  const uint32_t* words;
  uint32_t cell;
  if (!occ_locate(g, x, y, z, words, cell)) return g.outside != 0;
  return occ_bit(words, cell);
}

// (written out, not occ_locate + a load or a loop over occ_level: either moves instructions in the cascade's query / classify kernels,
// which keep the listing they had before the split -- tools/isa_funcs.py against the parent: 0 of its kernels differ)
__device__ __forceinline__ bool occ_point(const OccCascadeDev& c, float x, float y, float z) {
  for (int l = 0; l < c.levels; ++l) {
    const OccLevel& g = c.g[l];
    const float fi = floorf(fmul(fsub(x, g.lo[0]), g.inv[0]));
    const float fj = floorf(fmul(fsub(y, g.lo[1]), g.inv[1]));
    const float fk = floorf(fmul(fsub(z, g.lo[2]), g.inv[2]));
    // (& not &&: one straight-line test per level, its 40 bytes of geometry fetched by one batch of scalar loads)
    if ((fi >= 0.f) & (fi < (float)g.n[0]) & (fj >= 0.f) & (fj < (float)g.n[1]) & (fk >= 0.f) & (fk < (float)g.n[2]))
      return occ_bit(c.words[l], ((uint32_t)fi * (uint32_t)g.n[1] + (uint32_t)fj) * (uint32_t)g.n[2] + (uint32_t)fk);
  }
  return c.outside != 0;
}

// ---- host side ---------------------------------------------------------------------------------------------------
inline bool occ_dims(int64_t nx, int64_t ny, int64_t nz, OccDims* d) {
  if (nx < 1 || ny < 1 || nz < 1 || nx > (1 << 24) || ny > (1 << 24) || nz > (1 << 24)) return false;
  if (nx > (((int64_t)1 << 31) - 1) / ny / nz) return false;
  d->nx = (int)nx;
  d->ny = (int)ny;
  d->nz = (int)nz;
  d->ncells = nx * ny * nz;
  d->nwords = (d->ncells + 31) / 32;
  return true;
}

// the grid's geometry without its bits (o->words = g->words, which may be NULL)
inline bool occ_geom(const fn_occ_grid* g, OccDev* o) {
  OccDims d;
  if (!g || !occ_dims(g->n[0], g->n[1], g->n[2], &d)) return false;
  o->words = g->words;
  for (int c = 0; c < 3; ++c) {
    if (!(g->inv[c] > 0.f) || !(g->inv[c] <= 3.0e38f) || !(g->lo[c] == g->lo[c])) return false;
    o->lo[c] = g->lo[c];
    o->inv[c] = g->inv[c];
    o->n[c] = g->n[c];
  }
  o->outside = g->outside_occupied ? 1 : 0;
  return true;
}

inline bool occ_dev(const fn_occ_grid* g, OccDev* o) { return g && g->words && occ_geom(g, o); }

// every level passes occ_dev's checks; the cascade's `outside` is the LAST level's outside_occupied
inline bool occ_cascade_dev(const fn_occ_cascade* c, OccCascadeDev* o) {
  if (!c || c->levels < 1 || c->levels > FN_OCC_MAX_LEVELS) return false;
  *o = OccCascadeDev{};
  for (int l = 0; l < c->levels; ++l) {
    OccDev d;
    if (!occ_dev(&c->level[l], &d)) return false;
    for (int a = 0; a < 3; ++a) {
      o->g[l].lo[a] = d.lo[a];
      o->g[l].inv[a] = d.inv[a];
      o->g[l].n[a] = d.n[a];
    }
    o->words[l] = d.words;
    o->outside = d.outside;
  }
  o->levels = c->levels;
  return true;
}

}  // namespace
