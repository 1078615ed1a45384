// Gradient of the trilinear sample with respect to the sample POSITION: grid_sampler_3d_backward's other half (the
// grad_grid half is grid_sample.hip).  What camera-pose refinement differentiates through (ops.ray_points, pose.py).
//
// One lane per sample, both layouts.  The sample's cell, its per-axis weights and the in-range test are the gather's
// (dvgo_tri_setup / dvgo_tri_inb: same expressions, same bits); floorf chooses the cell, so on a lattice plane the
// derivative is the upper cell's, as in F.grid_sample's own backward.  Per channel c, ascending, the eight corners in the
// gather's order n = 0..7 (bit2 = +X, bit1 = +Y, bit0 = +Z), out-of-range corners skipped:
//     dX_c = fmaf(v, sx(n) * (wz * wy), dX_c)    dY_c = fmaf(v, sy(n) * (wz * wx), dY_c)    dZ_c = fmaf(v, sz(n) * (wy * wx), dZ_c)
// each from 0, the sign -1 on the lower corner of that axis and +1 on the upper (exact); then ax = fmaf(g[m,c], dX_c, ax)
// and, after the last channel, grad_xyz[m,0] = ax * ((float)(X-1) / (max[0] - min[0])); likewise y and z.
//
// The 8 (generic) or 8 x float4 (channels-last, C % 4 == 0, 16-byte aligned) corner loads of a channel group are issued
// unconditionally from clamped, always valid addresses before the first fmaf, so all of them are in flight together
// (common.h: dvgo_tri_value_c1 explains what the conditional form costs); a select drops the out-of-range ones, which
// leaves the accumulation order above untouched.  Every row of grad_xyz is written by its lane with plain stores: no
// atomics, no workspace, nothing to zero beforehand.
#include "xyz_corners.h"   // XyzCorners, dvgo_xyz_corners, DVGO_XYZ_CHANNEL: shared with march_raygrad.hip's dense kernels

template <int VEC>   // VEC = 4: channels-last with C % 4 == 0 and 16-B aligned bases; 1: generic (element strides)
__global__ void __launch_bounds__(DVGO_BLOCK)
grid_sample_bwd_xyz_kernel(const float* __restrict__ grid, int C, int X, int Y, int Z,
                           int64_t sC, int64_t sX, int64_t sY, int64_t sZ,
                           const float* __restrict__ grad_out, const float* __restrict__ xyz,
                           const float* __restrict__ xyz_min, const float* __restrict__ xyz_max, int64_t M,
                           float* __restrict__ grad_xyz) {
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  const float mnx = xyz_min[0], mny = xyz_min[1], mnz = xyz_min[2];
  const float mxx = xyz_max[0], mxy = xyz_max[1], mxz = xyz_max[2];
  const TriSetup t = dvgo_tri_setup(xyz[3 * m], xyz[3 * m + 1], xyz[3 * m + 2], mnx, mny, mnz, mxx, mxy, mxz, X, Y, Z);
  const XyzCorners k = dvgo_xyz_corners(t, X, Y, Z, sX, sY, sZ);
  float ax = 0.f, ay = 0.f, az = 0.f;
  if (VEC == 4) {
    for (int c = 0; c < C; c += 4) {
      float4 v[8];
#pragma unroll
      for (int n = 0; n < 8; ++n) v[n] = *reinterpret_cast<const float4*>(grid + k.off[n] + c);
      const float4 g = *reinterpret_cast<const float4*>(grad_out + m * C + c);
      // hipcc otherwise sinks each 16-byte load to its corner's fmaf (one round trip per corner); nothing crosses this
      __builtin_amdgcn_sched_barrier(0);
      DVGO_XYZ_CHANNEL(v[n].x, g.x);
      DVGO_XYZ_CHANNEL(v[n].y, g.y);
      DVGO_XYZ_CHANNEL(v[n].z, g.z);
      DVGO_XYZ_CHANNEL(v[n].w, g.w);
    }
  } else {
    for (int c = 0; c < C; ++c) {
      float v[8];
#pragma unroll
      for (int n = 0; n < 8; ++n) v[n] = grid[c * sC + k.off[n]];
      const float g = grad_out[m * C + c];
      DVGO_XYZ_CHANNEL(v[n], g);
    }
  }
  grad_xyz[3 * m + 0] = ax * ((float)(X - 1) / (mxx - mnx));
  grad_xyz[3 * m + 1] = ay * ((float)(Y - 1) / (mxy - mny));
  grad_xyz[3 * m + 2] = az * ((float)(Z - 1) / (mxz - mnz));
}

extern "C" {

int dvgo_grid_sample_bwd_xyz(const float* grid, int C, int X, int Y, int Z, int64_t sC, int64_t sX,
                             int64_t sY, int64_t sZ, const float* grad_out, const float* xyz,
                             const float* xyz_min, const float* xyz_max, int64_t M, float* grad_xyz, void* stream) {
  if (M < 0 || C < 0 || X <= 0 || Y <= 0 || Z <= 0) return DVGO_EINVAL;
  if (M == 0) return 0;
  if (!grid || !grad_out || !xyz || !xyz_min || !xyz_max || !grad_xyz) return DVGO_EINVAL;
  if (!dvgo_fits(M * (int64_t)(C > 0 ? C : 1))) return DVGO_ERANGE;
  hipStream_t s = (hipStream_t)stream;
  const bool vec = (sC == 1) && (C % 4 == 0) && (sX % 4 == 0) && (sY % 4 == 0) && (sZ % 4 == 0) &&
                   ((((uintptr_t)grid) & 15) == 0) && ((((uintptr_t)grad_out) & 15) == 0);
  if (vec)
    grid_sample_bwd_xyz_kernel<4><<<dvgo_blocks(M, DVGO_BLOCK), DVGO_BLOCK, 0, s>>>(
        grid, C, X, Y, Z, sC, sX, sY, sZ, grad_out, xyz, xyz_min, xyz_max, M, grad_xyz);
  else
    grid_sample_bwd_xyz_kernel<1><<<dvgo_blocks(M, DVGO_BLOCK), DVGO_BLOCK, 0, s>>>(
        grid, C, X, Y, Z, sC, sX, sY, sZ, grad_out, xyz, xyz_min, xyz_max, M, grad_xyz);
  DVGO_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
