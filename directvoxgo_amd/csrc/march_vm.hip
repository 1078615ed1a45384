// Fused ray march over the vector-matrix (VM) decomposed density of TensoRFVoxGO: march.hip's march_density and
// march_density_bwd with the trilinear read of a dense grid replaced by vm_density.hip's sum of plane value times line
// value.  include/dvgo_hip.h (the VM march block) is the contract.
//
//   march_vm_density      one wavefront per ray, lanes = 64 consecutive steps: position -> box test -> occupancy byte ->
//                         the 3R products as one fma chain (vmd_fwd_kernel's, through the same helpers: the bits of
//                         dvgo_vm_density_fwd at that position) -> alpha -> alpha filter -> transmittance carry with early
//                         stop -> weight filter -> ballot / popcount compaction into the ray's rec2 records.
//                         A chunk in which no lane survives box and mask skips the density loop (a wave-uniform branch), and
//                         a ray never touches a chunk behind its stop: what the op-by-op path pays for every occupied sample
//                         of every ray, this kernel pays only up to the surface.
//   march_vm_density_bwd  one wavefront per ray over its records from the far end: march_density_bwd's walk, chunk by
//                         chunk the same function (march_records.h: march_bwd_chunk); record i of ray r leaves its
//                         raw-density gradient at g_raw[off2[r] + i] and its position at xyz2[off2[r] + i].  No scatter, no
//                         atomics, no LDS: bitwise repeatable.  The scatter into planes and lines is dvgo_vm_density_bwd on
//                         (g_raw, xyz2), which passes over exact zeros.
//
// The records, dvgo_march_gather, dvgo_march_composite and their backward are march.hip's, unchanged.  The occupancy lookup
// (common.h: dvgo_mask_index), the activation (the alpha filter is one compare behind it, here as there), the transmittance
// carry -- the plain ballot / readlane walk of march_density_kernel's FAST == false body, not the hand-scheduled chain_walk --
// and the commit of a chunk into the records are the functions march.hip calls: march_records.h owns them.
#include "march_records.h"
#include "vm_common.h"

struct MarchVmParams {
  float mnx, mny, mnz, mxx, mxy, mxz;
  float stepdist;                       // > 0
  float scx, scy, scz, shx, shy, shz;   // xyz2ijk scale / shift
  int mX, mY, mZ;
  float act_shift, interval, thres;
};

__device__ __forceinline__ float mvm_axis(int a, float x, float y, float z) { return (a == 0) ? x : (a == 1) ? y : z; }

// VEC = 4: R % 4 == 0, channels-last, 16-byte aligned planes and lines; VEC = 1: everything else.  Same chain, same bits.
template <int VEC>
__global__ void __launch_bounds__(DVGO_BLOCK)
march_vm_density_kernel(TpPlane PA, TpPlane PB, TpPlane PC, VmLine LA, VmLine LB, VmLine LC, int R,
                        const float* __restrict__ rays_o, const float* __restrict__ rays_d, float near, float far,
                        float* __restrict__ rays_start, float* __restrict__ rays_dir, int64_t* __restrict__ n_steps,
                        int64_t rec_stride, int64_t n_rays, const uint8_t* __restrict__ mask, MarchVmParams P,
                        dvgo_rec2_t* __restrict__ rec2, int32_t* __restrict__ n2, int32_t* __restrict__ n3,
                        float* __restrict__ alphainv_last) {
  const int64_t ray = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (ray >= n_rays) return;
  // K1-K3 of this ray; lane 0 leaves the start point, the unit direction and the step count for the kernels behind
  const RaySetup S = dvgo_ray_setup(rays_o[3 * ray], rays_o[3 * ray + 1], rays_o[3 * ray + 2], rays_d[3 * ray], rays_d[3 * ray + 1],
                                    rays_d[3 * ray + 2], P.mnx, P.mny, P.mnz, P.mxx, P.mxy, P.mxz, near, far, P.stepdist);
  const float sx = S.sx, sy = S.sy, sz = S.sz, dx = S.dx, dy = S.dy, dz = S.dz;
  if (lane == 0) {
    n_steps[ray] = S.n;
    rays_start[3 * ray] = sx; rays_start[3 * ray + 1] = sy; rays_start[3 * ray + 2] = sz;
    rays_dir[3 * ray] = dx; rays_dir[3 * ray + 1] = dy; rays_dir[3 * ray + 2] = dz;
  }
  // the ray's records are [cs0, cs0 + rec_stride): a step count above the caller's bound is not marched past it
  const int ns = __builtin_amdgcn_readfirstlane((int)(S.n < rec_stride ? S.n : rec_stride));
  const int64_t cs0 = ray * rec_stride;
  const bool filt = P.thres > 0.0f;
  const unsigned long long lt = lanemask_lt(lane);

  float Tc = 1.0f;
  int c2 = 0, c3 = 0;
  for (int base = 0; base < ns; base += 64) {
    const int step = base + lane;
    const float dist = march_dist(P.stepdist, step);
    const float px = fmaf(dx, dist, sx), py = fmaf(dy, dist, sy), pz = fmaf(dz, dist, sz);
    bool keep = (step < ns) && !((P.mnx > px) | (P.mny > py) | (P.mnz > pz) | (P.mxx < px) | (P.mxy < py) | (P.mxz < pz));
    if (mask != nullptr && keep) {
      int64_t idx;
      keep = dvgo_mask_index(px, py, pz, P.scx, P.scy, P.scz, P.shx, P.shy, P.shz, P.mX, P.mY, P.mZ, idx);
      if (keep) keep = mask[idx] != 0;
    }
    if (__ballot(keep) == 0ull) continue;          // empty or masked-out chunk: no density loop, nothing to carry or record
    float e = 0.f, a = 0.f;
    if (keep) {
      float acc = 0.f;
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        int ah, aw, al;
        const TpPlane q = tp_pick(PA, PB, PC, s, ah, aw);
        const VmLine ln = vm_pick(LA, LB, LC, s, al);
        const float ph = mvm_axis(ah, px, py, pz), mnh = mvm_axis(ah, P.mnx, P.mny, P.mnz), mxh = mvm_axis(ah, P.mxx, P.mxy, P.mxz);
        const float pw = mvm_axis(aw, px, py, pz), mnw = mvm_axis(aw, P.mnx, P.mny, P.mnz), mxw = mvm_axis(aw, P.mxx, P.mxy, P.mxz);
        int n0;
        float w0, w1;
        tp_axis(dvgo_src_index(mvm_axis(al, px, py, pz), mvm_axis(al, P.mnx, P.mny, P.mnz), mvm_axis(al, P.mxx, P.mxy, P.mxz), ln.N),
                n0, w0, w1);
#pragma unroll 2
        for (int c = 0; c < R; c += VEC) {
          const TpVal<VEC> l = vm_line<VEC>(ln, c, n0, w0, w1);
          const TpVal<VEC> p = tp_sample<VEC>(q, c, ph, pw, mnh, mxh, mnw, mxw);
#pragma unroll
          for (int i = 0; i < VEC; ++i) acc = fmaf(p.v[i], l.v[i], acc);
        }
      }
      march_alpha(acc, P.act_shift, P.interval, e, a);
      if (filt) keep = a > P.thres;
    }
    // transmittance: the float carry walks the kept lanes only; then the stop cut, the weight filter and the records
    const double f = 1.0 - (double)a + 1e-10;
    float T_before = 1.0f;
    const int stop_lane = plain_walk(__ballot(keep), f, lane, Tc, T_before);
    const MarchCommit cm = march_commit(keep, stop_lane, step, e, a, T_before, filt, P.thres, lane, lt, rec2, cs0, c2, c3);
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
march_vm_density_bwd_kernel(const dvgo_rec2_t* __restrict__ rec2, const int32_t* __restrict__ n2, int64_t rec_stride,
                            const int64_t* __restrict__ off3, const int64_t* __restrict__ off2, int64_t n_rays,
                            const float* __restrict__ rays_start, const float* __restrict__ rays_dir, float stepdist,
                            const float* __restrict__ alphainv_last, float interval, const float* __restrict__ grad_weights,
                            const float* __restrict__ grad_last, float* __restrict__ g_raw, float* __restrict__ xyz2) {
  const int64_t ray = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (ray >= n_rays) return;
  const int c2 = __builtin_amdgcn_readfirstlane(n2[ray]);
  if (c2 == 0) return;
  const int64_t cs0 = ray * rec_stride;
  const int64_t o3 = off3[ray], o2 = off2[ray];
  const int c3_rem = (int)(off3[ray + 1] - o3);
  const float sx = rays_start[3 * ray], sy = rays_start[3 * ray + 1], sz = rays_start[3 * ray + 2];
  const float dx = rays_dir[3 * ray], dy = rays_dir[3 * ray + 1], dz = rays_dir[3 * ray + 2];
  const float acc = (grad_last ? grad_last[ray] : 0.0f) * alphainv_last[ray];
  march_records_bwd(rec2, c2, cs0, o3, c3_rem, o2, lane, acc, interval, grad_weights, g_raw, xyz2,
                    [&](int step, float& x, float& y, float& z) {
                      const float dist = march_dist(stepdist, step);
                      x = fmaf(dx, dist, sx); y = fmaf(dy, dist, sy); z = fmaf(dz, dist, sz);
                    });
}

extern "C" {

// NOTE: xyz_min / xyz_max / xyz2ijk_scale / xyz2ijk_shift are HOST pointers (3 floats each), as in march.hip's entries.

int dvgo_march_vm_density(float* rays_start, float* rays_dir, int64_t* n_steps, int64_t rec_stride, int64_t n_rays,
                          const float* xyz_min, const float* xyz_max, float stepdist,
                          const uint8_t* mask, int mX, int mY, int mZ, const float* xyz2ijk_scale, const float* xyz2ijk_shift,
                          const float* xy, int H_xy, int W_xy, int64_t sC_xy, int64_t sH_xy, int64_t sW_xy,
                          const float* yz, int H_yz, int W_yz, int64_t sC_yz, int64_t sH_yz, int64_t sW_yz,
                          const float* zx, int H_zx, int W_zx, int64_t sC_zx, int64_t sH_zx, int64_t sW_zx,
                          const float* l_xy, int N_xy, int64_t lC_xy, int64_t lN_xy,
                          const float* l_yz, int N_yz, int64_t lC_yz, int64_t lN_yz,
                          const float* l_zx, int N_zx, int64_t lC_zx, int64_t lN_zx,
                          int R, float act_shift, float interval, float fast_color_thres,
                          dvgo_rec2_t* rec2, int32_t* n2, int32_t* n3, float* alphainv_last,
                          const float* rays_o, const float* rays_d, float near, float far, void* stream) {
  const TpPlanes P = TP_PLANES(xy, yz, zx);
  const VmLines L = VM_LINES();
  // shapes first (vm_check's order), among them what this march does not do: NDC spacing, the exact record layout
  if (n_rays < 0 || R < 1 || !tp_plane_ok(P.a) || !tp_plane_ok(P.b) || !tp_plane_ok(P.c) || L.a.N < 1 || L.b.N < 1 || L.c.N < 1 ||
      !(stepdist > 0.0f) || rec_stride <= 0)
    return DVGO_EINVAL;
  if (n_rays == 0) return 0;
  if (!rays_start || !rays_dir || !n_steps || !xyz_min || !xyz_max || !P.a.p || !P.b.p || !P.c.p || !L.a.p || !L.b.p || !L.c.p ||
      !rec2 || !n2 || !n3 || !alphainv_last || !rays_o || !rays_d)
    return DVGO_EINVAL;
  if (mask && (!xyz2ijk_scale || !xyz2ijk_shift || mX <= 0 || mY <= 0 || mZ <= 0)) return DVGO_EINVAL;
  if (!dvgo_fits(n_rays * 64) || !dvgo_fits(rec_stride)) return DVGO_ERANGE;
  MarchVmParams Q;
  Q.mnx = xyz_min[0]; Q.mny = xyz_min[1]; Q.mnz = xyz_min[2];
  Q.mxx = xyz_max[0]; Q.mxy = xyz_max[1]; Q.mxz = xyz_max[2];
  Q.stepdist = stepdist;
  Q.scx = mask ? xyz2ijk_scale[0] : 0.f; Q.scy = mask ? xyz2ijk_scale[1] : 0.f; Q.scz = mask ? xyz2ijk_scale[2] : 0.f;
  Q.shx = mask ? xyz2ijk_shift[0] : 0.f; Q.shy = mask ? xyz2ijk_shift[1] : 0.f; Q.shz = mask ? xyz2ijk_shift[2] : 0.f;
  Q.mX = mX; Q.mY = mY; Q.mZ = mZ;
  Q.act_shift = act_shift; Q.interval = interval; Q.thres = fast_color_thres;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (R % 4 == 0) && tp_planes_vec(P, 4) && vm_line_vec(L.a) && vm_line_vec(L.b) && vm_line_vec(L.c);
  const int blocks = dvgo_blocks(n_rays * 64, DVGO_BLOCK);
  if (vec)
    march_vm_density_kernel<4><<<blocks, DVGO_BLOCK, 0, st>>>(P.a, P.b, P.c, L.a, L.b, L.c, R, rays_o, rays_d, near, far, rays_start,
                                                              rays_dir, n_steps, rec_stride, n_rays, mask, Q, rec2, n2, n3,
                                                              alphainv_last);
  else
    march_vm_density_kernel<1><<<blocks, DVGO_BLOCK, 0, st>>>(P.a, P.b, P.c, L.a, L.b, L.c, R, rays_o, rays_d, near, far, rays_start,
                                                              rays_dir, n_steps, rec_stride, n_rays, mask, Q, rec2, n2, n3,
                                                              alphainv_last);
  DVGO_LAUNCH_CHECK();
  return 0;
}

int dvgo_march_vm_density_bwd(const dvgo_rec2_t* rec2, const int32_t* n2, const int64_t* n_steps, int64_t rec_stride,
                              const int64_t* off3, const int64_t* off2, int64_t n_rays,
                              const float* rays_start, const float* rays_dir, float stepdist,
                              const float* alphainv_last, float interval,
                              const float* grad_weights, const float* grad_last,
                              float* g_raw, float* xyz2, void* stream) {
  if (n_rays < 0 || !(stepdist > 0.0f) || rec_stride <= 0) return DVGO_EINVAL;
  if (n_rays == 0) return 0;
  if (!rec2 || !n2 || !n_steps || !off3 || !off2 || !rays_start || !rays_dir || !alphainv_last || !g_raw || !xyz2)
    return DVGO_EINVAL;       // grad_weights may be NULL when M3 == 0 (it is only read for flagged records)
  if (!dvgo_fits(n_rays * 64)) return DVGO_ERANGE;
  march_vm_density_bwd_kernel<<<dvgo_blocks(n_rays * 64, DVGO_BLOCK), DVGO_BLOCK, 0, (hipStream_t)stream>>>(
      rec2, n2, rec_stride, off3, off2, n_rays, rays_start, rays_dir, stepdist, alphainv_last, interval, grad_weights, grad_last,
      g_raw, xyz2);
  DVGO_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
