// What the hash-grid translation units share (hashgrid.hip: the sampler and the scatter into the table; hash_xyz.hip: the
// sampler's gradient with respect to the position).  Device: the level table, the row type, the cell of a sample on a
// level (floor node and per-axis weights) and the row of a node.  Host: the level table's check, the alignment
// predicate and the dispatch over F.  include/dvgo_hip.h (the hash block) states the arithmetic.
#pragma once
#include "common.h"

struct HashLevels {
  int L;
  unsigned int hashed;                      // bit l: level l is hashed
  int rx[DVGO_HASH_MAX_LEVELS], ry[DVGO_HASH_MAX_LEVELS], rz[DVGO_HASH_MAX_LEVELS];
  unsigned int mask[DVGO_HASH_MAX_LEVELS];  // size_l - 1 of a hashed level
  long long off[DVGO_HASH_MAX_LEVELS];      // first row of the level
};

template <int F> struct __attribute__((aligned(F >= 4 ? 16 : 4 * F))) HashRow { float v[F]; };

// floor node and the two weights of one axis: the coordinate clamped into the lattice, so both nodes exist
__device__ __forceinline__ void hash_axis(float p, float mn, float mx, int R, int& f, float& w0, float& w1) {
  float g = dvgo_src_index(p, mn, mx, R);
  g = fminf(fmaxf(g, 0.0f), (float)(R - 1));       // (a NaN position lands on node 0: no address leaves the level)
  f = min((int)floorf(g), R - 2);
  const float ff = (float)f;
  w0 = (ff + 1.0f) - g;
  w1 = g - ff;
}

// the clamp of hash_axis is idle: the unclamped coordinate lies in [0, R - 1] (a NaN does not)
__device__ __forceinline__ bool hash_inside(float p, float mn, float mx, int R) {
  const float g = dvgo_src_index(p, mn, mx, R);
  return (g >= 0.0f) & (g <= (float)(R - 1));
}

struct HashCell { int fx, fy, fz; float wx[2], wy[2], wz[2]; };

__device__ __forceinline__ HashCell hash_cell(const HashLevels& LV, int l, const float* __restrict__ xyz,
                                              const float* __restrict__ mn, const float* __restrict__ mx, int64_t m) {
  HashCell c;
  hash_axis(xyz[3 * m + 0], mn[0], mx[0], LV.rx[l], c.fx, c.wx[0], c.wx[1]);
  hash_axis(xyz[3 * m + 1], mn[1], mx[1], LV.ry[l], c.fy, c.wy[0], c.wy[1]);
  hash_axis(xyz[3 * m + 2], mn[2], mx[2], LV.rz[l], c.fz, c.wz[0], c.wz[1]);
  return c;
}

// row of node (ix, iy, iz) of level l in the table (the level's offset included)
__device__ __forceinline__ int64_t hash_row(const HashLevels& LV, int l, bool hashed, int ix, int iy, int iz) {
  const int64_t dense = ((int64_t)ix * LV.ry[l] + iy) * LV.rz[l] + iz;
  const unsigned int h = ((unsigned int)ix * 1u ^ (unsigned int)iy * 2654435761u ^ (unsigned int)iz * 805459861u) & LV.mask[l];
  return LV.off[l] + (hashed ? (int64_t)h : dense);
}

// < 0: the error; 0: the level table is valid and filled in
static int hash_levels(int F, int L, const int32_t* res, const int64_t* offsets, HashLevels& LV) {
  if (!(F == 1 || F == 2 || F == 4 || F == 8) || L < 1 || L > DVGO_HASH_MAX_LEVELS || !res || !offsets) return DVGO_EINVAL;
  if (offsets[0] < 0) return DVGO_EINVAL;
  LV.L = L;
  LV.hashed = 0u;
  for (int l = 0; l < DVGO_HASH_MAX_LEVELS; ++l) {
    LV.rx[l] = LV.ry[l] = LV.rz[l] = 2;
    LV.mask[l] = 0u;
    LV.off[l] = 0;
  }
  for (int l = 0; l < L; ++l) {
    const int64_t rx = res[3 * l + 0], ry = res[3 * l + 1], rz = res[3 * l + 2];
    if (rx < 2 || ry < 2 || rz < 2) return DVGO_EINVAL;
    if (rx * ry >= ((int64_t)1 << 31)) return DVGO_ERANGE;          // the node count below then fits int64
    const int64_t nodes = rx * ry * rz;
    const int64_t size = offsets[l + 1] - offsets[l];
    if (size < 1) return DVGO_EINVAL;
    if (size != nodes) {
      if (size > nodes || (size & (size - 1)) != 0) return DVGO_EINVAL;
      if (size > ((int64_t)1 << 31)) return DVGO_ERANGE;
      LV.hashed |= 1u << l;
      LV.mask[l] = (unsigned int)(size - 1);
    }
    LV.rx[l] = (int)rx; LV.ry[l] = (int)ry; LV.rz[l] = (int)rz;
    LV.off[l] = offsets[l];
  }
  return 0;
}

static bool hash_aligned(const void* p, int F) { return (((uintptr_t)p) & (uintptr_t)(F >= 4 ? 15 : 4 * F - 1)) == 0; }

#define HASH_BY_F(F, LAUNCH)   \
  switch (F) {                 \
    case 1: LAUNCH(1); break;  \
    case 2: LAUNCH(2); break;  \
    case 4: LAUNCH(4); break;  \
    default: LAUNCH(8); break; \
  }
