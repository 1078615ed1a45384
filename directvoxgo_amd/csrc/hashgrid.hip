// Multiresolution hash-grid features (Mueller et al., Instant-NGP, SIGGRAPH 2022): L levels of a trilinear lattice whose
// nodes are rows of one table [T_total, F], a level either dense (one row per node) or hashed into a power-of-two number
// of rows; and the gradient scatter into the table.  include/dvgo_hip.h (the hash block) states the arithmetic.
//
// Forward: a lane owns (sample, level): the eight rows are addressed first and loaded unconditionally (every corner exists:
// the coordinate is clamped into the lattice), F floats each as one load of 4 F bytes, then the fma chains run.  Level is
// the fastest lane index, so a wave's stores are 64 consecutive pieces of `out` and the 64 lanes read 64 / L positions.
//
// Backward: the gradient is linear in the table, so nothing of the table is read.  Unmerged, a sample adds 8 L F dwords, on a
// hashed level into eight unrelated rows: the scattered shape that float atomics run slowest at.
//   mode 1  a lane owns (a run of consecutive samples, level), keeps the 8 F corner sums of the cell it is in in registers
//           and issues its atomics when the cell changes and at the end of its run: consecutive samples of a ray share the
//           cell on every level coarser than the march step.  Level fastest, as in the forward: grad_out is read in
//           consecutive pieces.
//   mode 2  nothing merged: a lane owns (sample, level, corner) and adds its F floats; the eight lanes of a cell sit side by
//           side, so the two z-neighbours of a dense level form one contiguous piece.
//   mode 3  mode 1 with the F channels of a row on F neighbouring lanes: a lane owns (run, level, channel) and keeps eight
//           sums; one atomic wave-instruction then adds whole rows of 4 F contiguous bytes, 64 / F rows instead of 64.
#include "hash_common.h"   // HashLevels, HashRow, hash_cell, hash_row, hash_levels, hash_aligned, HASH_BY_F: shared with hash_xyz.hip

// mode 0's choice and the run length a lane merges by default, from the A/B of profiles/hash/README.md: at L = 16, F = 2,
// 2^19 rows per hashed level and 2 097 152 samples in ray order mode 1 took 28.4 / 15.9 / 14.0 / 13.1 / 12.6 ms at run
// 1 / 4 / 8 / 16 / 32, mode 3 14.2 / 8.0 / 7.0 / 6.5 / 6.3 ms and mode 2 17.1 ms; at L = 8, F = 4 mode 3 took 3.2 ms at run
// 32 against mode 1's 13.0: the time follows the number of rows a wave-instruction touches, 64 / F in mode 3.  The same
// order on the sparse scene's 202 763 samples.
#define HASH_MODE_DEFAULT 3
#define HASH_RUN_DEFAULT 32

// corner n of the cell: bit 2 = +x, bit 1 = +y, bit 0 = +z (x slowest, z fastest)
__device__ __forceinline__ float hash_weight(const HashCell& c, int n) {
  return (c.wx[(n >> 2) & 1] * c.wy[(n >> 1) & 1]) * c.wz[n & 1];
}

// total = M * L lanes (< 2^31: the entry checks M * L * F)
template <int F>
__global__ void __launch_bounds__(DVGO_BLOCK)
hash_fwd_kernel(const float* __restrict__ table, HashLevels LV, const float* __restrict__ xyz, const float* __restrict__ mn,
                const float* __restrict__ mx, unsigned int total, float* __restrict__ out) {
  const unsigned int tid = blockIdx.x * (unsigned int)DVGO_BLOCK + threadIdx.x;
  if (tid >= total) return;
  const unsigned int m = tid / (unsigned int)LV.L;
  const int l = (int)(tid - m * (unsigned int)LV.L);
  const bool hashed = (LV.hashed >> l) & 1u;
  const HashCell c = hash_cell(LV, l, xyz, mn, mx, m);
  HashRow<F> r[8];
#pragma unroll
  for (int n = 0; n < 8; ++n) {
    const int64_t row = hash_row(LV, l, hashed, c.fx + ((n >> 2) & 1), c.fy + ((n >> 1) & 1), c.fz + (n & 1));
    r[n] = *reinterpret_cast<const HashRow<F>*>(table + row * F);
  }
  HashRow<F> o;
#pragma unroll
  for (int i = 0; i < F; ++i) o.v[i] = 0.f;
#pragma unroll
  for (int n = 0; n < 8; ++n) {
    const float w = hash_weight(c, n);
#pragma unroll
    for (int i = 0; i < F; ++i) o.v[i] = fmaf(r[n].v[i], w, o.v[i]);
  }
  *reinterpret_cast<HashRow<F>*>(out + (int64_t)tid * F) = o;
}

template <int F>
__device__ __forceinline__ void hash_flush(float* __restrict__ grad, const HashLevels& LV, int l, bool hashed, int fx, int fy,
                                           int fz, const float (&acc)[8][F]) {
#pragma unroll
  for (int n = 0; n < 8; ++n) {
    float* p = grad + hash_row(LV, l, hashed, fx + ((n >> 2) & 1), fy + ((n >> 1) & 1), fz + (n & 1)) * F;
#pragma unroll
    for (int i = 0; i < F; ++i) atomicAdd(p + i, acc[n][i]);
  }
}

// mode 1.  total = nchunk * L lanes, nchunk = ceil(M / run); lane (chunk, l) walks the samples [chunk * run, min(+run, M))
template <int F>
__global__ void __launch_bounds__(DVGO_BLOCK)
hash_bwd_run_kernel(float* __restrict__ grad, HashLevels LV, const float* __restrict__ grad_out, const float* __restrict__ xyz,
                    const float* __restrict__ mn, const float* __restrict__ mx, int64_t M, int run, int64_t total) {
  const int64_t tid = (int64_t)blockIdx.x * DVGO_BLOCK + threadIdx.x;
  if (tid >= total) return;
  const int64_t chunk = tid / LV.L;
  const int l = (int)(tid - chunk * LV.L);
  const bool hashed = (LV.hashed >> l) & 1u;
  const int64_t m0 = chunk * run;
  const int64_t m1 = (m0 + run < M) ? m0 + run : M;
  int cx = INT_MIN, cy = INT_MIN, cz = INT_MIN;
  float acc[8][F];
  for (int64_t m = m0; m < m1; ++m) {
    const HashCell c = hash_cell(LV, l, xyz, mn, mx, m);
    const HashRow<F> g = *reinterpret_cast<const HashRow<F>*>(grad_out + (m * LV.L + l) * F);
    if ((c.fx != cx) | (c.fy != cy) | (c.fz != cz)) {
      if (cx != INT_MIN) hash_flush<F>(grad, LV, l, hashed, cx, cy, cz, acc);
      cx = c.fx; cy = c.fy; cz = c.fz;
#pragma unroll
      for (int n = 0; n < 8; ++n)
#pragma unroll
        for (int i = 0; i < F; ++i) acc[n][i] = 0.f;
    }
#pragma unroll
    for (int n = 0; n < 8; ++n) {
      const float w = hash_weight(c, n);
#pragma unroll
      for (int i = 0; i < F; ++i) acc[n][i] += w * g.v[i];
    }
  }
  if (cx != INT_MIN) hash_flush<F>(grad, LV, l, hashed, cx, cy, cz, acc);
}

// mode 3.  total = nchunk * L * F lanes, channel fastest, then level; lane (chunk, l, c) walks the samples of its chunk
template <int F>
__global__ void __launch_bounds__(DVGO_BLOCK)
hash_bwd_chan_kernel(float* __restrict__ grad, HashLevels LV, const float* __restrict__ grad_out, const float* __restrict__ xyz,
                     const float* __restrict__ mn, const float* __restrict__ mx, int64_t M, int run, int64_t total) {
  const int64_t tid = (int64_t)blockIdx.x * DVGO_BLOCK + threadIdx.x;
  if (tid >= total) return;
  const int c = (int)(tid % F);
  const int64_t cl = tid / F;
  const int64_t chunk = cl / LV.L;
  const int l = (int)(cl - chunk * LV.L);
  const bool hashed = (LV.hashed >> l) & 1u;
  const int64_t m0 = chunk * run;
  const int64_t m1 = (m0 + run < M) ? m0 + run : M;
  int cx = INT_MIN, cy = INT_MIN, cz = INT_MIN;
  float acc[8];
  for (int64_t m = m0; m < m1; ++m) {
    const HashCell cell = hash_cell(LV, l, xyz, mn, mx, m);
    const float g = grad_out[(m * LV.L + l) * F + c];
    if ((cell.fx != cx) | (cell.fy != cy) | (cell.fz != cz)) {
      if (cx != INT_MIN) {
#pragma unroll
        for (int n = 0; n < 8; ++n)
          atomicAdd(grad + hash_row(LV, l, hashed, cx + ((n >> 2) & 1), cy + ((n >> 1) & 1), cz + (n & 1)) * F + c, acc[n]);
      }
      cx = cell.fx; cy = cell.fy; cz = cell.fz;
#pragma unroll
      for (int n = 0; n < 8; ++n) acc[n] = 0.f;
    }
#pragma unroll
    for (int n = 0; n < 8; ++n) acc[n] += hash_weight(cell, n) * g;
  }
  if (cx != INT_MIN) {
#pragma unroll
    for (int n = 0; n < 8; ++n)
      atomicAdd(grad + hash_row(LV, l, hashed, cx + ((n >> 2) & 1), cy + ((n >> 1) & 1), cz + (n & 1)) * F + c, acc[n]);
  }
}

// mode 2.  total = M * L * 8 lanes (< 2^31: the entry checks), corner fastest, then level
template <int F>
__global__ void __launch_bounds__(DVGO_BLOCK)
hash_bwd_corner_kernel(float* __restrict__ grad, HashLevels LV, const float* __restrict__ grad_out, const float* __restrict__ xyz,
                       const float* __restrict__ mn, const float* __restrict__ mx, unsigned int total) {
  const unsigned int tid = blockIdx.x * (unsigned int)DVGO_BLOCK + threadIdx.x;
  if (tid >= total) return;
  const int n = (int)(tid & 7u);
  const unsigned int ml = tid >> 3;
  const unsigned int m = ml / (unsigned int)LV.L;
  const int l = (int)(ml - m * (unsigned int)LV.L);
  const bool hashed = (LV.hashed >> l) & 1u;
  const HashCell c = hash_cell(LV, l, xyz, mn, mx, m);
  const HashRow<F> g = *reinterpret_cast<const HashRow<F>*>(grad_out + (int64_t)ml * F);
  const float w = hash_weight(c, n);
  float* p = grad + hash_row(LV, l, hashed, c.fx + ((n >> 2) & 1), c.fy + ((n >> 1) & 1), c.fz + (n & 1)) * F;
#pragma unroll
  for (int i = 0; i < F; ++i) atomicAdd(p + i, w * g.v[i]);
}

extern "C" {

int dvgo_hash_fwd(const float* table, int F, int L, const int32_t* res, const int64_t* offsets, const float* xyz,
                  const float* xyz_min, const float* xyz_max, int64_t M, float* out, void* stream) {
  HashLevels LV;
  const int rc = hash_levels(F, L, res, offsets, LV);
  if (rc < 0) return rc;
  if (M < 0) return DVGO_EINVAL;
  if (M == 0) return 0;
  if (!table || !xyz || !xyz_min || !xyz_max || !out || !hash_aligned(table, F) || !hash_aligned(out, F)) return DVGO_EINVAL;
  if (!dvgo_fits(M * L * (int64_t)F)) return DVGO_ERANGE;
  hipStream_t st = (hipStream_t)stream;
  const unsigned int total = (unsigned int)(M * L);
  const int blocks = dvgo_blocks(total, DVGO_BLOCK);
#define HASH_LAUNCH(FF) hash_fwd_kernel<FF><<<blocks, DVGO_BLOCK, 0, st>>>(table, LV, xyz, xyz_min, xyz_max, total, out)
  HASH_BY_F(F, HASH_LAUNCH)
#undef HASH_LAUNCH
  DVGO_LAUNCH_CHECK();
  return 0;
}

int dvgo_hash_bwd(const float* grad_out, float* grad_table, int F, int L, const int32_t* res, const int64_t* offsets,
                  const float* xyz, const float* xyz_min, const float* xyz_max, int64_t M, int run, int mode, void* stream) {
  HashLevels LV;
  const int rc = hash_levels(F, L, res, offsets, LV);
  if (rc < 0) return rc;
  if (M < 0 || run < 0 || mode < 0 || mode > 3) return DVGO_EINVAL;
  if (M == 0) return 0;
  if (!grad_out || !grad_table || !xyz || !xyz_min || !xyz_max || !hash_aligned(grad_out, F) || !hash_aligned(grad_table, F))
    return DVGO_EINVAL;
  if (!dvgo_fits(M * L * (int64_t)F)) return DVGO_ERANGE;
  if (mode == 0) mode = HASH_MODE_DEFAULT;
  if (mode == 2 && !dvgo_fits(M * L * 8)) return DVGO_ERANGE;
  hipStream_t st = (hipStream_t)stream;
  if (mode == 2) {
    const unsigned int total = (unsigned int)(M * L * 8);
    const int blocks = dvgo_blocks(total, DVGO_BLOCK);
#define HASH_LAUNCH(FF) \
  hash_bwd_corner_kernel<FF><<<blocks, DVGO_BLOCK, 0, st>>>(grad_table, LV, grad_out, xyz, xyz_min, xyz_max, total)
    HASH_BY_F(F, HASH_LAUNCH)
#undef HASH_LAUNCH
  } else if (mode == 3) {
    if (run == 0) run = HASH_RUN_DEFAULT;
    const int64_t nchunk = (M + run - 1) / run;
    const int64_t total = nchunk * L * F;                          // <= M L F: fits
    const int blocks = dvgo_blocks(total, DVGO_BLOCK);
#define HASH_LAUNCH(FF) \
  hash_bwd_chan_kernel<FF><<<blocks, DVGO_BLOCK, 0, st>>>(grad_table, LV, grad_out, xyz, xyz_min, xyz_max, M, run, total)
    HASH_BY_F(F, HASH_LAUNCH)
#undef HASH_LAUNCH
  } else {
    if (run == 0) run = HASH_RUN_DEFAULT;
    const int64_t nchunk = (M + run - 1) / run;
    const int64_t total = nchunk * L;
    const int blocks = dvgo_blocks(total, DVGO_BLOCK);
#define HASH_LAUNCH(FF) \
  hash_bwd_run_kernel<FF><<<blocks, DVGO_BLOCK, 0, st>>>(grad_table, LV, grad_out, xyz, xyz_min, xyz_max, M, run, total)
    HASH_BY_F(F, HASH_LAUNCH)
#undef HASH_LAUNCH
  }
  DVGO_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
