// Gradient of the multiresolution hash-grid features with respect to the sample POSITION: what camera-pose refinement
// differentiates through when the colour features come from a hash table (ops.hash_sample(position_grad=True),
// HashVoxGO(raygrad=True), pose.py).  The table's own gradient is hashgrid.hip.  include/dvgo_hip.h (the hash block)
// states the arithmetic.
//
// One lane per sample, the levels in a loop, l ascending.  On a level the cell and the per-axis weights are the forward's
// (hash_cell: same expressions, same bits), so the derivative is that of the cell the forward chose: the upper cell on an
// interior lattice plane, the last cell at g == R - 1.  Where the forward's clamp acts on an axis the features do not
// depend on that coordinate, and the level adds exactly 0.0f along it (hash_inside, judged on the unclamped coordinate: a
// NaN is outside).  Every row of grad_xyz is written by its lane with plain stores: no atomics, no workspace, nothing to
// zero beforehand.
//
// Why this mapping and not the forward's (sample, level) lanes.  The three outputs of a sample are sums over its L levels
// and have to come out in one fixed order.  With a lane per (sample, level) that is a reduction over L neighbouring lanes
// which, L being any number up to 32, straddle waves: LDS, a barrier and a second pass, or a DPP chain with a tail case,
// to add L numbers.  Here the sum is a register and its order is the loop's.  What the forward's mapping buys, the number
// of row loads in flight, is the same here per wave -- the 8 rows of a level, 4 F bytes each (two 16-byte loads at
// F = 8), issued from always valid addresses before the first fmaf -- and at the sizes the op sees (10^5 - 10^6 samples,
// thousands of waves) the machine is full either way.  What it costs: a lane reads its grad_out piece of 4 F bytes at a
// stride of 4 L F bytes from its neighbour's, so a wave's load of grad_out touches 64 cache lines where the forward's
// store touches 4 F; the pieces of a sample are consecutive, so a line fetched for one level serves the levels after it.
// The level loop indexes the level table (a kernel argument) by a wave-uniform l: scalar loads, no private memory.
#include "hash_common.h"

template <int F>
__global__ void __launch_bounds__(DVGO_BLOCK)
hash_bwd_xyz_kernel(const float* __restrict__ table, HashLevels LV, const float* __restrict__ grad_out,
                    const float* __restrict__ xyz, const float* __restrict__ mn, const float* __restrict__ mx, int64_t M,
                    float* __restrict__ grad_xyz) {
  const int64_t m = (int64_t)blockIdx.x * DVGO_BLOCK + threadIdx.x;
  if (m >= M) return;
  const float px = xyz[3 * m + 0], py = xyz[3 * m + 1], pz = xyz[3 * m + 2];
  const float mnx = mn[0], mny = mn[1], mnz = mn[2];
  const float mxx = mx[0], mxy = mx[1], mxz = mx[2];
  float ox = 0.f, oy = 0.f, oz = 0.f;
  for (int l = 0; l < LV.L; ++l) {
    const bool hashed = (LV.hashed >> l) & 1u;
    const HashCell c = hash_cell(LV, l, xyz, mn, mx, m);
    HashRow<F> r[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) {
      const int64_t row = hash_row(LV, l, hashed, c.fx + ((n >> 2) & 1), c.fy + ((n >> 1) & 1), c.fz + (n & 1));
      r[n] = *reinterpret_cast<const HashRow<F>*>(table + row * F);
    }
    const HashRow<F> g = *reinterpret_cast<const HashRow<F>*>(grad_out + (m * LV.L + l) * F);
    // hipcc otherwise sinks each row load to its corner's fmaf (one round trip per corner); nothing crosses this
    __builtin_amdgcn_sched_barrier(0);
    // signed two-weight products of corner n: d/dx pairs (wy, wz), d/dy (wx, wz), d/dz (wx, wy); the sign is exact
    float sx[8], sy[8], sz[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) {
      const int bx = (n >> 2) & 1, by = (n >> 1) & 1, bz = n & 1;
      const float yz = c.wy[by] * c.wz[bz], xz = c.wx[bx] * c.wz[bz], xy = c.wx[bx] * c.wy[by];
      sx[n] = bx ? yz : -yz;
      sy[n] = by ? xz : -xz;
      sz[n] = bz ? xy : -xy;
    }
    float ax = 0.f, ay = 0.f, az = 0.f;
#pragma unroll
    for (int i = 0; i < F; ++i) {
      float dx = 0.f, dy = 0.f, dz = 0.f;
#pragma unroll
      for (int n = 0; n < 8; ++n) {
        dx = fmaf(r[n].v[i], sx[n], dx);
        dy = fmaf(r[n].v[i], sy[n], dy);
        dz = fmaf(r[n].v[i], sz[n], dz);
      }
      ax = fmaf(g.v[i], dx, ax);
      ay = fmaf(g.v[i], dy, ay);
      az = fmaf(g.v[i], dz, az);
    }
    const int Rx = LV.rx[l], Ry = LV.ry[l], Rz = LV.rz[l];
    const float tx = ax * ((float)(Rx - 1) / (mxx - mnx));
    const float ty = ay * ((float)(Ry - 1) / (mxy - mny));
    const float tz = az * ((float)(Rz - 1) / (mxz - mnz));
    ox = ox + (hash_inside(px, mnx, mxx, Rx) ? tx : 0.0f);
    oy = oy + (hash_inside(py, mny, mxy, Ry) ? ty : 0.0f);
    oz = oz + (hash_inside(pz, mnz, mxz, Rz) ? tz : 0.0f);
  }
  grad_xyz[3 * m + 0] = ox;
  grad_xyz[3 * m + 1] = oy;
  grad_xyz[3 * m + 2] = oz;
}

extern "C" {

int dvgo_hash_bwd_xyz(const float* table, int F, int L, const int32_t* res, const int64_t* offsets, const float* grad_out,
                      const float* xyz, const float* xyz_min, const float* xyz_max, int64_t M, float* grad_xyz, void* stream) {
  HashLevels LV;
  const int rc = hash_levels(F, L, res, offsets, LV);
  if (rc < 0) return rc;
  if (M < 0) return DVGO_EINVAL;
  if (M == 0) return 0;
  if (!table || !grad_out || !xyz || !xyz_min || !xyz_max || !grad_xyz || !hash_aligned(table, F) || !hash_aligned(grad_out, F))
    return DVGO_EINVAL;
  if (!dvgo_fits(M * L * (int64_t)F)) return DVGO_ERANGE;
  hipStream_t st = (hipStream_t)stream;
  const int blocks = dvgo_blocks(M, DVGO_BLOCK);
#define HASH_LAUNCH(FF) \
  hash_bwd_xyz_kernel<FF><<<blocks, DVGO_BLOCK, 0, st>>>(table, LV, grad_out, xyz, xyz_min, xyz_max, M, grad_xyz)
  HASH_BY_F(F, HASH_LAUNCH)
#undef HASH_LAUNCH
  DVGO_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
