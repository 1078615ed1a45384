// The corner table of the trilinear sample's POSITION derivative, shared by grid_sample_xyz.hip (one lane per sample) and
// march_raygrad.hip's dense kernels (one lane per record of a ray): signed two-weight products, clamped offsets, in-range
// flags, and the per-channel corner chains.  include/dvgo_hip.h (dvgo_grid_sample_bwd_xyz) states the arithmetic.
#pragma once
#include "common.h"

struct XyzCorners {
  float wx[8], wy[8], wz[8];   // signed two-weight products of corner n for d/dx, d/dy, d/dz
  int64_t off[8];              // element offset of the clamped corner (channel 0)
  bool ok[8];                  // corner inside the lattice
};

__device__ __forceinline__ XyzCorners dvgo_xyz_corners(const TriSetup& t, int X, int Y, int Z, int64_t sX, int64_t sY, int64_t sZ) {
  XyzCorners k;
#pragma unroll
  for (int n = 0; n < 8; ++n) {
    const float wz = (n & 1) ? t.wz1 : t.wz0;
    const float wy = (n & 2) ? t.wy1 : t.wy0;
    const float wx = (n & 4) ? t.wx1 : t.wx0;
    const float zy = wz * wy, zx = wz * wx, yx = wy * wx;
    k.wx[n] = (n & 4) ? zy : -zy;
    k.wy[n] = (n & 2) ? zx : -zx;
    k.wz[n] = (n & 1) ? yx : -yx;
    k.ok[n] = dvgo_tri_inb(t, n, X, Y, Z);
    const int i = min(max(t.i0 + ((n >> 2) & 1), 0), X - 1);
    const int j = min(max(t.j0 + ((n >> 1) & 1), 0), Y - 1);
    const int kk = min(max(t.k0 + (n & 1), 0), Z - 1);
    k.off[n] = (int64_t)i * sX + (int64_t)j * sY + (int64_t)kk * sZ;
  }
  return k;
}

// one channel: the three corner chains from 0, then the channel's term of the three sums (reads the XyzCorners `k`,
// accumulates into `ax`, `ay`, `az` of the enclosing scope)
#define DVGO_XYZ_CHANNEL(V, G)                                           \
  do {                                                                   \
    float dx = 0.f, dy = 0.f, dz = 0.f;                                  \
    _Pragma("unroll") for (int n = 0; n < 8; ++n) {                      \
      const float v_ = (V);                                              \
      dx = k.ok[n] ? fmaf(v_, k.wx[n], dx) : dx;                         \
      dy = k.ok[n] ? fmaf(v_, k.wy[n], dy) : dy;                         \
      dz = k.ok[n] ? fmaf(v_, k.wz[n], dz) : dz;                         \
    }                                                                    \
    ax = fmaf((G), dx, ax);                                              \
    ay = fmaf((G), dy, ay);                                              \
    az = fmaf((G), dz, az);                                              \
  } while (0)
