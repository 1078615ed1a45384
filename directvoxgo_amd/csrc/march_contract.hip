// Fused ray march over the contracted space of DirectContractedVoxGO: contract.hip's sampler and march.hip's march_density
// in one kernel, step per lane.  include/dvgo_hip.h (the contracted march block) is the contract.
//
//   march_contract_density      one wavefront per ray, lanes = 64 consecutive steps k of the table t_tab: point -> norm ->
//                               contraction q_k -> segment length ||q_k - q_{k-1}|| (contract_common.h: the sampler's float32
//                               expressions) -> thinning -> occupancy byte -> density trilinear at q_k over the contracted bounds
//                               (march_density_kernel's read: the bits of dvgo_grid_sample_fwd) -> alpha -> alpha filter ->
//                               transmittance carry with early stop -> weight filter -> ballot / popcount compaction into the
//                               ray's rec2 records (rec_stride = n_max is always a bound).
//                               The thinning (acc += d_k; over = acc > thres; acc = 0 when over) is a recurrence with reset: it
//                               is resolved in step order over the chunk's lanes by a readlane walk, the same float32 adds in the
//                               same order as the sampler's, and acc is carried from chunk to chunk.  The walk runs in every
//                               chunk up to the ray's stop; a chunk in which no lane is kept skips the density read, the
//                               transmittance carry and the records (a wave-uniform branch), and nothing behind the stop is
//                               visited: what the op-by-op path pays twice for all n_max steps of every ray, and then for every
//                               occupied sample, this kernel pays only up to the surface.
//   march_contract_density_bwd  one wavefront per ray over its records from the far end (march_records.h: march_records_bwd, the
//                               walk of march_vm_density_bwd, on march_density_bwd's chunk); record i of ray r leaves its raw-density
//                               gradient at g_raw[off2[r] + i] and its contracted position at q2[off2[r] + i].  No scatter, no
//                               atomics, no LDS: bitwise repeatable.  The scatter into the grid is dvgo_grid_sample_bwd (C = 1).
//   contract_positions          elementwise: q and t of kept (ray, step) pairs, the bits dvgo_contract_emit writes for them
//                               (dvgo_march_gather rebuilds positions of uniform steps only; here it runs with no feature grid).
//
// The records, dvgo_march_gather, dvgo_march_composite and their backward are march.hip's, unchanged.  The activation
// (the alpha filter is one compare behind it, here as there), the transmittance carry -- the plain ballot / readlane walk of
// march_density_kernel's FAST == false body, not the hand-scheduled chain_walk -- and the commit of a chunk into the records
// are the functions march.hip calls: march_records.h owns them, as common.h's dvgo_mask_index owns the occupancy lookup
// behind contract_occupied.
#include "contract_common.h"
#include "march_records.h"

struct MarchContractParams {
  float cx, cy, cz, rx, ry, rz;         // centre and radius of the foreground box
  float b, thin;                        // bg_len; the thinning distance
  int l2;
  float mnx, mny, mnz, mxx, mxy, mxz;   // contracted bounds of the grids
  float scx, scy, scz, shx, shy, shz;   // xyz2ijk scale / shift of the occupancy mask
  int mX, mY, mZ;
  int X, Y, Z;
  float act_shift, interval, thres;
};

__global__ void __launch_bounds__(DVGO_BLOCK)
march_contract_density_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d, int64_t n_rays,
                              const float* __restrict__ t_tab, int n_max, int64_t rec_stride,
                              const uint8_t* __restrict__ mask, const float* __restrict__ density, MarchContractParams P,
                              dvgo_rec2_t* __restrict__ rec2, int32_t* __restrict__ n2, int32_t* __restrict__ n3,
                              float* __restrict__ alphainv_last) {
  const int64_t ray = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (ray >= n_rays) return;
  const ContractRay R = contract_ray(rays_o, rays_d, ray, P.cx, P.cy, P.cz, P.rx, P.ry, P.rz);
  const float one_b = 1.0f + P.b;
  const int64_t cs0 = ray * rec_stride;
  const int64_t YZ = (int64_t)P.Y * P.Z;
  const bool filt = P.thres > 0.0f;
  const bool pairs = P.Z >= 2;
  const unsigned long long lt = lanemask_lt(lane);

  float lqx = 0.0f, lqy = 0.0f, lqz = 0.0f;      // q of the step before this chunk (q_k is a pure function of (ray, k): carried)
  float acc = 0.0f;                              // the thinning's accumulated distance: wave-uniform, carried
  float Tc = 1.0f;
  int c2 = 0, c3 = 0;
  for (int base = 0; base < n_max; base += 64) {
    const int k = base + lane;
    const bool live = k < n_max;
    const float t = t_tab[live ? k : n_max - 1];
    float qx, qy, qz;
    const bool inner = contract_point(R, t, P.b, one_b, P.l2, qx, qy, qz);
    float ux = __shfl_up(qx, 1), uy = __shfl_up(qy, 1), uz = __shfl_up(qz, 1);
    if (lane == 0) { ux = lqx; uy = lqy; uz = lqz; }
    const float d = contract_segment(qx, qy, qz, ux, uy, uz);
    lqx = dvgo_readlane_f(qx, 63); lqy = dvgo_readlane_f(qy, 63); lqz = dvgo_readlane_f(qz, 63);
    // thinning, in step order: the sampler's `acc = acc + d_k; over = acc > thres; if (over) acc = 0` for k > 0
    unsigned long long over_m = 0ull;
    const int nv = min(64, n_max - base);
    for (int j = (base == 0) ? 1 : 0; j < nv; ++j) {
      acc = acc + dvgo_readlane_f(d, j);
      if (acc > P.thin) { over_m |= 1ull << j; acc = 0.0f; }
    }
    const bool over = (over_m >> lane) & 1ull;
    bool keep = live && (inner || over);
    if (keep && mask != nullptr) {
      // dvgo_march_contract_density answers DVGO_EINVAL for a mask with mZ <= 0 before it launches (its `if (mask && ...)`
      // check below): said here, the index product needs no sign word of mZ.  The assumption goes if that check ever does.
      __builtin_assume(P.mZ > 0);
      keep = contract_occupied(qx, qy, qz, mask, P.mX, P.mY, P.mZ, P.scx, P.scy, P.scz, P.shx, P.shy, P.shz);
    }
    if (__ballot(keep) == 0ull) continue;         // nothing kept: no density read, nothing to carry or record
    float e = 0.f, a = 0.f;
    if (keep) {
      const TriSetup s = dvgo_tri_setup(qx, qy, qz, P.mnx, P.mny, P.mnz, P.mxx, P.mxy, P.mxz, P.X, P.Y, P.Z);
      float dn = 0.f;
      if (pairs) {
        dn = dvgo_tri_value_c1(density, s, P.X, P.Y, P.Z);
      } else {
#pragma unroll
        for (int n = 0; n < 8; ++n) {
          if (dvgo_tri_inb(s, n, P.X, P.Y, P.Z)) {
            const int64_t off = (int64_t)(s.i0 + ((n >> 2) & 1)) * YZ + (int64_t)(s.j0 + ((n >> 1) & 1)) * P.Z + (s.k0 + (n & 1));
            dn = fmaf(density[off], dvgo_tri_weight(s, n), dn);
          }
        }
      }
      march_alpha(dn, P.act_shift, P.interval, e, a);
      if (filt) keep = a > P.thres;
    }
    // transmittance: the float carry walks the kept lanes only; then the stop cut, the weight filter and the records
    // (a ray writes at most n_max <= rec_stride of them)
    const double f = 1.0 - (double)a + 1e-10;
    float T_before = 1.0f;
    const int stop_lane = plain_walk(__ballot(keep), f, lane, Tc, T_before);
    const MarchCommit cm = march_commit(keep, stop_lane, k, e, a, T_before, filt, P.thres, lane, lt, rec2, cs0, c2, c3);
    c2 = cm.c2; c3 = cm.c3;
    if (stop_lane >= 0) break;
  }
  if (lane == 0) {
    n2[ray] = c2;
    n3[ray] = c3;
    alphainv_last[ray] = Tc;
  }
}

__global__ void __launch_bounds__(DVGO_BLOCK)
march_contract_density_bwd_kernel(const dvgo_rec2_t* __restrict__ rec2, const int32_t* __restrict__ n2, int64_t rec_stride,
                                  const int64_t* __restrict__ off3, const int64_t* __restrict__ off2, int64_t n_rays,
                                  const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                  const float* __restrict__ t_tab, int n_max, MarchContractParams P,
                                  const float* __restrict__ alphainv_last, const float* __restrict__ grad_weights,
                                  const float* __restrict__ grad_last, float* __restrict__ g_raw, float* __restrict__ q2) {
  const int64_t ray = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (ray >= n_rays) return;
  const int c2 = __builtin_amdgcn_readfirstlane(n2[ray]);
  if (c2 == 0) return;
  const int64_t cs0 = ray * rec_stride;
  const int64_t o3 = off3[ray], o2 = off2[ray];
  const int c3_rem = (int)(off3[ray + 1] - o3);
  const ContractRay R = contract_ray(rays_o, rays_d, ray, P.cx, P.cy, P.cz, P.rx, P.ry, P.rz);
  const float one_b = 1.0f + P.b;
  const float acc = (grad_last ? grad_last[ray] : 0.0f) * alphainv_last[ray];
  march_records_bwd(rec2, c2, cs0, o3, c3_rem, o2, lane, acc, P.interval, grad_weights, g_raw, q2,
                    [&](int step, float& x, float& y, float& z) {
                      contract_point(R, t_tab[min(step, n_max - 1)], P.b, one_b, P.l2, x, y, z);
                    });
}

__global__ void __launch_bounds__(DVGO_BLOCK)
contract_positions_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d, int64_t n_rays,
                          const float* __restrict__ t_tab, int n_max, MarchContractParams P,
                          const int64_t* __restrict__ ray_id, const int64_t* __restrict__ step_id, int64_t M,
                          float* __restrict__ q, float* __restrict__ t_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const int64_t r = ray_id[i], k = step_id[i];
  float t = __int_as_float(0x7fc00000), qx = t, qy = t, qz = t;      // an id outside its range reads nothing and leaves NaN
  if (r >= 0 && r < n_rays && k >= 0 && k < n_max) {
    const ContractRay R = contract_ray(rays_o, rays_d, r, P.cx, P.cy, P.cz, P.rx, P.ry, P.rz);
    t = t_tab[k];
    contract_point(R, t, P.b, 1.0f + P.b, P.l2, qx, qy, qz);
  }
  q[3 * i] = qx; q[3 * i + 1] = qy; q[3 * i + 2] = qz;
  t_out[i] = t;
}

static MarchContractParams mc_params(const float* center, const float* radius, float bg_len, int l2, float thin) {
  MarchContractParams P = {};
  P.cx = center[0]; P.cy = center[1]; P.cz = center[2];
  P.rx = radius[0]; P.ry = radius[1]; P.rz = radius[2];
  P.b = bg_len; P.l2 = l2; P.thin = thin;
  return P;
}

extern "C" {

// NOTE: center / radius / xyz_min / xyz_max / xyz2ijk_scale / xyz2ijk_shift are HOST pointers (3 floats each), as in march.hip's
// entries.

int dvgo_march_contract_density(const float* rays_o, const float* rays_d, int64_t n_rays, const float* center,
                                const float* radius, const float* t_tab, int n_max, float bg_len, int l2, float thin_thres,
                                const uint8_t* mask, int mX, int mY, int mZ, const float* xyz2ijk_scale,
                                const float* xyz2ijk_shift, const float* density, int X, int Y, int Z, const float* xyz_min,
                                const float* xyz_max, float act_shift, float interval, float fast_color_thres,
                                int64_t rec_stride, dvgo_rec2_t* rec2, int32_t* n2, int32_t* n3, float* alphainv_last,
                                void* stream) {
  if (n_rays < 0 || n_max <= 0 || X <= 0 || Y <= 0 || Z <= 0 || rec_stride < n_max) return DVGO_EINVAL;
  if (n_rays == 0) return 0;
  if (!rays_o || !rays_d || !center || !radius || !t_tab || !density || !xyz_min || !xyz_max || !rec2 || !n2 || !n3 ||
      !alphainv_last)
    return DVGO_EINVAL;
  if (mask && (!xyz2ijk_scale || !xyz2ijk_shift || mX <= 0 || mY <= 0 || mZ <= 0)) return DVGO_EINVAL;
  if (!dvgo_fits(n_rays * 64) || !dvgo_fits(rec_stride) || !dvgo_fits((int64_t)X * Y * Z)) return DVGO_ERANGE;
  MarchContractParams P = mc_params(center, radius, bg_len, l2, thin_thres);
  P.mnx = xyz_min[0]; P.mny = xyz_min[1]; P.mnz = xyz_min[2];
  P.mxx = xyz_max[0]; P.mxy = xyz_max[1]; P.mxz = xyz_max[2];
  if (mask) {
    P.scx = xyz2ijk_scale[0]; P.scy = xyz2ijk_scale[1]; P.scz = xyz2ijk_scale[2];
    P.shx = xyz2ijk_shift[0]; P.shy = xyz2ijk_shift[1]; P.shz = xyz2ijk_shift[2];
  }
  P.mX = mX; P.mY = mY; P.mZ = mZ;
  P.X = X; P.Y = Y; P.Z = Z;
  P.act_shift = act_shift; P.interval = interval; P.thres = fast_color_thres;
  march_contract_density_kernel<<<dvgo_blocks(n_rays * 64, DVGO_BLOCK), DVGO_BLOCK, 0, (hipStream_t)stream>>>(
      rays_o, rays_d, n_rays, t_tab, n_max, rec_stride, mask, density, P, rec2, n2, n3, alphainv_last);
  DVGO_LAUNCH_CHECK();
  return 0;
}

int dvgo_march_contract_density_bwd(const dvgo_rec2_t* rec2, const int32_t* n2, int64_t rec_stride, const int64_t* off3,
                                    const int64_t* off2, int64_t n_rays, const float* rays_o, const float* rays_d,
                                    const float* center, const float* radius, const float* t_tab, int n_max, float bg_len,
                                    int l2, const float* alphainv_last, float interval, const float* grad_weights,
                                    const float* grad_last, float* g_raw, float* q2, void* stream) {
  if (n_rays < 0 || n_max <= 0 || rec_stride < n_max) return DVGO_EINVAL;
  if (n_rays == 0) return 0;
  if (!rec2 || !n2 || !off3 || !off2 || !rays_o || !rays_d || !center || !radius || !t_tab || !alphainv_last || !g_raw || !q2)
    return DVGO_EINVAL;       // grad_weights may be NULL when M3 == 0 (it is only read for flagged records)
  if (!dvgo_fits(n_rays * 64) || !dvgo_fits(rec_stride)) return DVGO_ERANGE;
  MarchContractParams P = mc_params(center, radius, bg_len, l2, 0.0f);
  P.interval = interval;
  march_contract_density_bwd_kernel<<<dvgo_blocks(n_rays * 64, DVGO_BLOCK), DVGO_BLOCK, 0, (hipStream_t)stream>>>(
      rec2, n2, rec_stride, off3, off2, n_rays, rays_o, rays_d, t_tab, n_max, P, alphainv_last, grad_weights, grad_last, g_raw,
      q2);
  DVGO_LAUNCH_CHECK();
  return 0;
}

int dvgo_contract_positions(const float* rays_o, const float* rays_d, int64_t n_rays, const float* center,
                            const float* radius, const float* t_tab, int n_max, float bg_len, int l2,
                            const int64_t* ray_id, const int64_t* step_id, int64_t M, float* q, float* t, void* stream) {
  if (n_rays < 0 || M < 0 || n_max <= 0) return DVGO_EINVAL;
  if (M == 0) return 0;
  if (!rays_o || !rays_d || !center || !radius || !t_tab || !ray_id || !step_id || !q || !t) return DVGO_EINVAL;
  if (!dvgo_fits(M) || !dvgo_fits(n_rays)) return DVGO_ERANGE;
  const MarchContractParams P = mc_params(center, radius, bg_len, l2, 0.0f);
  contract_positions_kernel<<<dvgo_blocks(M, DVGO_BLOCK), DVGO_BLOCK, 0, (hipStream_t)stream>>>(
      rays_o, rays_d, n_rays, t_tab, n_max, P, ray_id, step_id, M, q, t);
  DVGO_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
