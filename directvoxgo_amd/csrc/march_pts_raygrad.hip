// The ray gradient of the fused marches that hand POSITIONS to their caller (camera-pose refinement on the fused path of
// HashVoxGO, VMTriPlaneVoxGO and TensoRFVoxGO; pose.py).  Two siblings of march.hip's
// march_ray_bwd_kernel, which differentiates a march whose colour features are a k0 grid:
//
//   march_pts_ray_bwd     the dense density grid (fused_march(positions=True)): march_ray_bwd_kernel with the k0 term
//                         replaced by the gradient that arrived for the kept samples' positions,
//                             g_p = scale * (g_d * d density / d g)  +  [kept] grad_pts[off3[ray] + rank]
//   march_vm_ray_bwd      the decomposed density (fused_march_vm): the same walk over the records of march_vm_density,
//                             g_p = g_raw * d(sum_{s,r} plane_{s,r} * line_{s,r}) / d xyz  +  [kept] grad_pts[off3[ray] + rank]
//                         with the position derivative of vm_xyz.hip's vm_bwd_xyz_kernel<VEC, false>: its cell, weights,
//                         dropped corners and nodes, component order and per-plane scale, on the helpers that kernel calls.
//
// Both: one wavefront per ray; the ray's rec2 records from the far end in chunks of 64 through march_bwd_chunk
// (march_records.h: the walk of every march backward); the record's position from the forward's expression
// fmaf(dir, march_dist(stepdist, step), start), hence its bits; lam = t_min + dist / |d| a constant of the derivative;
//     grad_o[ray] = sum g_p        grad_d[ray] = sum lam * g_p
// in float32, a butterfly over the 64 lanes per chunk (lanes without a record add 0), chunks far to near into one
// accumulator per component.  Lane 0 writes both rows with plain stores, zeros for a ray without records: no atomics, no
// LDS, no workspace, nothing to zero beforehand, bitwise repeatable.  Neither kernel reads what the density backward of
// its march leaves behind (g_raw, xyz2): each does its own walk, so a frozen model, whose density backward never runs,
// still moves its cameras.  include/dvgo_hip.h states the arithmetic.
#include "march_records.h"
#include "vm_common.h"
#include "xyz_corners.h"

// (march.hip's, which that unit keeps to itself: the per-chunk butterfly and where a ray's records start)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

__device__ __forceinline__ int64_t rec_base(const int64_t* __restrict__ cum, const int64_t* __restrict__ n_steps,
                                            int64_t rec_stride, int64_t ray) {
  return cum ? (cum[ray] - n_steps[ray]) : ray * rec_stride;
}

struct PtsParams {
  float mnx, mny, mnz, mxx, mxy, mxz;
  float stepdist;          // > 0
  int X, Y, Z;             // the density lattice (the dense kernel only)
  float interval;
};

__device__ __forceinline__ float pts_axis(int a, float x, float y, float z) { return (a == 0) ? x : (a == 1) ? y : z; }

__global__ void __launch_bounds__(DVGO_BLOCK)
march_pts_ray_bwd_kernel(const dvgo_rec2_t* __restrict__ rec2, const int32_t* __restrict__ n2,
                         const int64_t* __restrict__ n_steps, const int64_t* __restrict__ cum, int64_t rec_stride,
                         const int64_t* __restrict__ off3, int64_t n_rays, const float* __restrict__ rays_start,
                         const float* __restrict__ rays_dir, PtsParams P, const float* __restrict__ alphainv_last,
                         const float* __restrict__ rays_o, const float* __restrict__ rays_d, float near, float far,
                         const float* __restrict__ density, const float* __restrict__ grad_weights,
                         const float* __restrict__ grad_last, const float* __restrict__ grad_pts,
                         float* __restrict__ grad_o, float* __restrict__ grad_d) {
  const int64_t ray = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (ray >= n_rays) return;
  const int c2 = __builtin_amdgcn_readfirstlane(n2[ray]);
  float Ax = 0.f, Ay = 0.f, Az = 0.f, Bx = 0.f, By = 0.f, Bz = 0.f;
  if (c2 > 0) {
    const int64_t cs0 = rec_base(cum, n_steps, rec_stride, ray);
    const int64_t o3 = off3[ray];
    int c3_rem = (int)(off3[ray + 1] - o3);
    const float sx = rays_start[3 * ray], sy = rays_start[3 * ray + 1], sz = rays_start[3 * ray + 2];
    const float dx = rays_dir[3 * ray], dy = rays_dir[3 * ray + 1], dz = rays_dir[3 * ray + 2];
    const RaySetup R = dvgo_ray_setup(rays_o[3 * ray], rays_o[3 * ray + 1], rays_o[3 * ray + 2], rays_d[3 * ray], rays_d[3 * ray + 1],
                                      rays_d[3 * ray + 2], P.mnx, P.mny, P.mnz, P.mxx, P.mxy, P.mxz, near, far, P.stepdist);
    const int64_t YZ = (int64_t)P.Y * P.Z;
    const float scale_x = (float)(P.X - 1) / (P.mxx - P.mnx);
    const float scale_y = (float)(P.Y - 1) / (P.mxy - P.mny);
    const float scale_z = (float)(P.Z - 1) / (P.mxz - P.mnz);
    const unsigned long long lt = lanemask_lt(lane);
    float acc = (grad_last ? grad_last[ray] : 0.0f) * alphainv_last[ray];
    for (int hi = c2; hi > 0; hi -= 64) {
      const int lo = max(0, hi - 64);
      const MarchBwdChunk ck = march_bwd_chunk(rec2, cs0, lo, hi - lo, lane, lt, o3, c3_rem, acc, grad_weights);
      const bool act = ck.act, flag = ck.flag;
      const int step = ck.step, rank = ck.rank;
      float gx = 0.f, gy = 0.f, gz = 0.f, lam = 0.f;
      if (act) {
        const float g_d = ck.g_d(P.interval);
        const float dist = march_dist(P.stepdist, step);
        const float px = fmaf(dx, dist, sx), py = fmaf(dy, dist, sy), pz = fmaf(dz, dist, sz);
        const TriSetup t = dvgo_tri_setup(px, py, pz, P.mnx, P.mny, P.mnz, P.mxx, P.mxy, P.mxz, P.X, P.Y, P.Z);
        const bool pts = flag && grad_pts != nullptr;
        if (g_d != 0.0f || pts) {            // (else: exact zeros, no loads)
          const XyzCorners k = dvgo_xyz_corners(t, P.X, P.Y, P.Z, YZ, (int64_t)P.Z, 1);
          float ax = 0.f, ay = 0.f, az = 0.f;
          float qx = 0.f, qy = 0.f, qz = 0.f;
          {
            float dv[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) dv[c] = density[k.off[c]];
            if (pts) {                       // the record's row of the positions' gradient, in flight with the corners
              const float* __restrict__ grow = grad_pts + (o3 + rank) * 3;
              qx = grow[0]; qy = grow[1]; qz = grow[2];
            }
            __builtin_amdgcn_sched_barrier(0);
            DVGO_XYZ_CHANNEL(dv[n], g_d);
          }
          gx = ax * scale_x; gy = ay * scale_y; gz = az * scale_z;
          if (pts) { gx = gx + qx; gy = gy + qy; gz = gz + qz; }
          lam = R.tmin + dist / R.rnorm;
        }
      }
      Ax += wave_sum(gx); Ay += wave_sum(gy); Az += wave_sum(gz);
      Bx += wave_sum(lam * gx); By += wave_sum(lam * gy); Bz += wave_sum(lam * gz);
    }
  }
  if (lane == 0) {
    grad_o[3 * ray] = Ax; grad_o[3 * ray + 1] = Ay; grad_o[3 * ray + 2] = Az;
    grad_d[3 * ray] = Bx; grad_d[3 * ray + 1] = By; grad_d[3 * ray + 2] = Bz;
  }
}

// VEC = 4: R % 4 == 0, channels-last, 16-byte aligned planes and lines (march_vm_density's rule); VEC = 1: everything
// else.  Same chains, same bits.
template <int VEC>
__global__ void __launch_bounds__(DVGO_BLOCK)
march_vm_ray_bwd_kernel(TpPlane PA, TpPlane PB, TpPlane PC, VmLine LA, VmLine LB, VmLine LC, int R,
                        const dvgo_rec2_t* __restrict__ rec2, const int32_t* __restrict__ n2, int64_t rec_stride,
                        const int64_t* __restrict__ off3, int64_t n_rays, const float* __restrict__ rays_start,
                        const float* __restrict__ rays_dir, PtsParams P, const float* __restrict__ alphainv_last,
                        const float* __restrict__ rays_o, const float* __restrict__ rays_d, float near, float far,
                        const float* __restrict__ grad_weights, const float* __restrict__ grad_last,
                        const float* __restrict__ grad_pts, float* __restrict__ grad_o, float* __restrict__ grad_d) {
  const int64_t ray = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (ray >= n_rays) return;
  const int c2 = __builtin_amdgcn_readfirstlane(n2[ray]);
  float* __restrict__ out_o = grad_o + 3 * ray;
  float* __restrict__ out_d = grad_d + 3 * ray;
  asm volatile("" : "+v"(out_o), "+v"(out_d));
  float Ax = 0.f, Ay = 0.f, Az = 0.f, Bx = 0.f, By = 0.f, Bz = 0.f;
  if (c2 > 0) {
    const int64_t o3 = off3[ray];
    int c3_rem = (int)(off3[ray + 1] - o3);
    // The ray's own rows as per-lane addresses, formed once: three planes and three lines by value leave few scalar
    // registers, and five base pointers held in them across the walk were spilled.  (march_bwd_chunk then gets 0 offsets.)
    const dvgo_rec2_t* __restrict__ recs = rec2 + ray * rec_stride;
    const float* __restrict__ gws = grad_weights + o3;
    const float* __restrict__ gps = grad_pts + 3 * o3;
    const bool has_pts = grad_pts != nullptr;
    asm volatile("" : "+v"(recs), "+v"(gws), "+v"(gps));
    // Likewise the 15 strides of planes and lines (30 scalar registers): they only ever multiply a lane's own corner or
    // node index, so they live in vector registers from here on.  Same values, same selects (tp_pick, vm_pick).
    TpPlane QA = PA, QB = PB, QC = PC;
    VmLine MA = LA, MB = LB, MC = LC;
    asm volatile("" : "+v"(QA.sC), "+v"(QA.sH), "+v"(QA.sW), "+v"(QB.sC), "+v"(QB.sH), "+v"(QB.sW), "+v"(QC.sC), "+v"(QC.sH),
                 "+v"(QC.sW));
    asm volatile("" : "+v"(MA.sC), "+v"(MA.sN), "+v"(MB.sC), "+v"(MB.sN), "+v"(MC.sC), "+v"(MC.sN));
    const float sx = rays_start[3 * ray], sy = rays_start[3 * ray + 1], sz = rays_start[3 * ray + 2];
    const float dx = rays_dir[3 * ray], dy = rays_dir[3 * ray + 1], dz = rays_dir[3 * ray + 2];
    const RaySetup S = dvgo_ray_setup(rays_o[3 * ray], rays_o[3 * ray + 1], rays_o[3 * ray + 2], rays_d[3 * ray], rays_d[3 * ray + 1],
                                      rays_d[3 * ray + 2], P.mnx, P.mny, P.mnz, P.mxx, P.mxy, P.mxz, near, far, P.stepdist);
    const unsigned long long lt = lanemask_lt(lane);
    float acc = (grad_last ? grad_last[ray] : 0.0f) * alphainv_last[ray];
    for (int hi = c2; hi > 0; hi -= 64) {
      const int lo = max(0, hi - 64);
      const MarchBwdChunk ck = march_bwd_chunk(recs, 0, lo, hi - lo, lane, lt, 0, c3_rem, acc, gws);
      const bool act = ck.act, flag = ck.flag;
      const int step = ck.step, rank = ck.rank;
      float gx = 0.f, gy = 0.f, gz = 0.f, lam = 0.f;
      if (act) {
        const float g_raw = ck.g_d(P.interval);
        const float dist = march_dist(P.stepdist, step);
        const float px = fmaf(dx, dist, sx), py = fmaf(dy, dist, sy), pz = fmaf(dz, dist, sz);
        const bool pts = flag && has_pts;
        if (g_raw != 0.0f || pts) {          // (else: the record is passed over)
          float qx = 0.f, qy = 0.f, qz = 0.f;
          if (pts) {
            const float* __restrict__ grow = gps + rank * 3;
            qx = grow[0]; qy = grow[1]; qz = grow[2];
          }
          float ox = 0.f, oy = 0.f, oz = 0.f;
          if (g_raw != 0.0f) {
            // vm_bwd_xyz_kernel<VEC, false> at p, the incoming gradient g_raw
#pragma unroll
            for (int s = 0; s < 3; ++s) {
              int ah, aw, al;
              const TpPlane q = tp_pick(QA, QB, QC, s, ah, aw);
              const VmLine ln = vm_pick(MA, MB, MC, s, al);
              const float mnh = pts_axis(ah, P.mnx, P.mny, P.mnz), mxh = pts_axis(ah, P.mxx, P.mxy, P.mxz);
              const float mnw = pts_axis(aw, P.mnx, P.mny, P.mnz), mxw = pts_axis(aw, P.mxx, P.mxy, P.mxz);
              const float mnl = pts_axis(al, P.mnx, P.mny, P.mnz), mxl = pts_axis(al, P.mxx, P.mxy, P.mxz);
              const BiSetup b = tp_setup(pts_axis(ah, px, py, pz), pts_axis(aw, px, py, pz), mnh, mxh, mnw, mxw, q.H, q.W);
              int n0;
              float w0, w1;
              tp_axis(dvgo_src_index(pts_axis(al, px, py, pz), mnl, mxl, ln.N), n0, w0, w1);
              const float k00 = b.wh0 * b.ww0, k01 = b.wh0 * b.ww1, k10 = b.wh1 * b.ww0, k11 = b.wh1 * b.ww1;
              float Ah = 0.f, Aw = 0.f, An = 0.f;
              for (int c = 0; c < R; c += VEC) {
                const VmNodes<VEC> nd = vm_gather<VEC>(ln, c, n0);
                const TpCorners<VEC> k = tp_gather<VEC>(q, b, c);
                // the four corners and two nodes of the group in flight together (vm_xyz.hip: nothing crosses this)
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                  const float l = vm_blend<VEC>(nd, i, w0, w1);
                  const float p = tp_blend<VEC>(k, i, k00, k01, k10, k11);
                  float dh = 0.f, dw = 0.f;
                  dh = (k.okh0 & k.okw0) ? fmaf(k.v00.v[i], -b.ww0, dh) : dh;
                  dh = (k.okh0 & k.okw1) ? fmaf(k.v01.v[i], -b.ww1, dh) : dh;
                  dh = (k.okh1 & k.okw0) ? fmaf(k.v10.v[i], b.ww0, dh) : dh;
                  dh = (k.okh1 & k.okw1) ? fmaf(k.v11.v[i], b.ww1, dh) : dh;
                  dw = (k.okh0 & k.okw0) ? fmaf(k.v00.v[i], -b.wh0, dw) : dw;
                  dw = (k.okh0 & k.okw1) ? fmaf(k.v01.v[i], b.wh0, dw) : dw;
                  dw = (k.okh1 & k.okw0) ? fmaf(k.v10.v[i], -b.wh1, dw) : dw;
                  dw = (k.okh1 & k.okw1) ? fmaf(k.v11.v[i], b.wh1, dw) : dw;
                  const float dn = (nd.ok1 ? nd.v1.v[i] : 0.f) - (nd.ok0 ? nd.v0.v[i] : 0.f);
                  const float t = g_raw * l, u = g_raw * p;
                  Ah = fmaf(t, dh, Ah);
                  Aw = fmaf(t, dw, Aw);
                  An = fmaf(u, dn, An);
                }
              }
              // the plane's scale once, after its last component; (ah, aw, al) is a permutation of the world axes
              const float th = Ah * ((float)(q.H - 1) / (mxh - mnh));
              const float tw = Aw * ((float)(q.W - 1) / (mxw - mnw));
              const float tn = An * ((float)(ln.N - 1) / (mxl - mnl));
              ox = ox + ((ah == 0) ? th : (aw == 0) ? tw : tn);
              oy = oy + ((ah == 1) ? th : (aw == 1) ? tw : tn);
              oz = oz + ((ah == 2) ? th : (aw == 2) ? tw : tn);
            }
          }
          gx = ox; gy = oy; gz = oz;
          if (pts) { gx = gx + qx; gy = gy + qy; gz = gz + qz; }
          lam = S.tmin + dist / S.rnorm;
        }
      }
      Ax += wave_sum(gx); Ay += wave_sum(gy); Az += wave_sum(gz);
      Bx += wave_sum(lam * gx); By += wave_sum(lam * gy); Bz += wave_sum(lam * gz);
    }
  }
  if (lane == 0) {
    out_o[0] = Ax; out_o[1] = Ay; out_o[2] = Az;
    out_d[0] = Bx; out_d[1] = By; out_d[2] = Bz;
  }
}

static PtsParams pts_params(const float* mn, const float* mx, float stepdist, int X, int Y, int Z, float interval) {
  PtsParams P;
  P.mnx = mn[0]; P.mny = mn[1]; P.mnz = mn[2];
  P.mxx = mx[0]; P.mxy = mx[1]; P.mxz = mx[2];
  P.stepdist = stepdist;
  P.X = X; P.Y = Y; P.Z = Z;
  P.interval = interval;
  return P;
}

extern "C" {

// NOTE: xyz_min / xyz_max are HOST pointers (3 floats each), as in march.hip's and march_vm.hip's entries.

int dvgo_march_ray_bwd_pts(const dvgo_rec2_t* rec2, const int32_t* n2, const int64_t* n_steps,
                           const int64_t* n_steps_cumsum, int64_t rec_stride, const int64_t* off3, int64_t n_rays,
                           const float* rays_start, const float* rays_dir, float stepdist,
                           const float* xyz_min, const float* xyz_max, const float* alphainv_last, float interval,
                           const float* rays_o, const float* rays_d, float near, float far,
                           const float* density, int X, int Y, int Z,
                           const float* grad_weights, const float* grad_last, const float* grad_pts,
                           float* grad_o, float* grad_d, void* stream) {
  if (n_rays < 0 || X <= 0 || Y <= 0 || Z <= 0 || !(stepdist > 0.0f)) return DVGO_EINVAL;   // NDC spacing is not differentiated
  if (n_rays == 0) return 0;
  if (!rec2 || !n2 || !n_steps || !off3 || !rays_start || !rays_dir || !xyz_min || !xyz_max || !alphainv_last ||
      !rays_o || !rays_d || !density || !grad_o || !grad_d)
    return DVGO_EINVAL;       // grad_weights may be NULL when M3 == 0 (it is only read for flagged records), grad_pts: no second term
  if (!n_steps_cumsum && rec_stride <= 0) return DVGO_EINVAL;
  if (!dvgo_fits(n_rays * 64)) return DVGO_ERANGE;
  const PtsParams P = pts_params(xyz_min, xyz_max, stepdist, X, Y, Z, interval);
  march_pts_ray_bwd_kernel<<<dvgo_blocks(n_rays * 64, DVGO_BLOCK), DVGO_BLOCK, 0, (hipStream_t)stream>>>(
      rec2, n2, n_steps, n_steps_cumsum, rec_stride, off3, n_rays, rays_start, rays_dir, P, alphainv_last, rays_o, rays_d,
      near, far, density, grad_weights, grad_last, grad_pts, grad_o, grad_d);
  DVGO_LAUNCH_CHECK();
  return 0;
}

int dvgo_march_vm_ray_bwd(const dvgo_rec2_t* rec2, const int32_t* n2, int64_t rec_stride, const int64_t* off3,
                          int64_t n_rays, const float* rays_start, const float* rays_dir, float stepdist,
                          const float* xyz_min, const float* xyz_max, const float* alphainv_last, float interval,
                          const float* rays_o, const float* rays_d, float near, float far,
                          const float* xy, int H_xy, int W_xy, int64_t sC_xy, int64_t sH_xy, int64_t sW_xy,
                          const float* yz, int H_yz, int W_yz, int64_t sC_yz, int64_t sH_yz, int64_t sW_yz,
                          const float* zx, int H_zx, int W_zx, int64_t sC_zx, int64_t sH_zx, int64_t sW_zx,
                          const float* l_xy, int N_xy, int64_t lC_xy, int64_t lN_xy,
                          const float* l_yz, int N_yz, int64_t lC_yz, int64_t lN_yz,
                          const float* l_zx, int N_zx, int64_t lC_zx, int64_t lN_zx,
                          int R, const float* grad_weights, const float* grad_last, const float* grad_pts,
                          float* grad_o, float* grad_d, void* stream) {
  const TpPlanes Q = TP_PLANES(xy, yz, zx);
  const VmLines L = VM_LINES();
  // shapes first (dvgo_march_vm_density's order), among them what its march does not do: NDC spacing, the exact record layout
  if (n_rays < 0 || R < 1 || !tp_plane_ok(Q.a) || !tp_plane_ok(Q.b) || !tp_plane_ok(Q.c) || L.a.N < 1 || L.b.N < 1 || L.c.N < 1 ||
      !(stepdist > 0.0f) || rec_stride <= 0)
    return DVGO_EINVAL;
  if (n_rays == 0) return 0;
  if (!rec2 || !n2 || !off3 || !rays_start || !rays_dir || !xyz_min || !xyz_max || !alphainv_last || !rays_o || !rays_d ||
      !Q.a.p || !Q.b.p || !Q.c.p || !L.a.p || !L.b.p || !L.c.p || !grad_o || !grad_d)
    return DVGO_EINVAL;       // grad_weights may be NULL when M3 == 0, grad_last and grad_pts when there is none
  if (!dvgo_fits(n_rays * 64) || !dvgo_fits(rec_stride)) return DVGO_ERANGE;
  const PtsParams P = pts_params(xyz_min, xyz_max, stepdist, 0, 0, 0, interval);
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (R % 4 == 0) && tp_planes_vec(Q, 4) && vm_line_vec(L.a) && vm_line_vec(L.b) && vm_line_vec(L.c);
  const int blocks = dvgo_blocks(n_rays * 64, DVGO_BLOCK);
  if (vec)
    march_vm_ray_bwd_kernel<4><<<blocks, DVGO_BLOCK, 0, st>>>(Q.a, Q.b, Q.c, L.a, L.b, L.c, R, rec2, n2, rec_stride, off3, n_rays,
                                                              rays_start, rays_dir, P, alphainv_last, rays_o, rays_d, near, far,
                                                              grad_weights, grad_last, grad_pts, grad_o, grad_d);
  else
    march_vm_ray_bwd_kernel<1><<<blocks, DVGO_BLOCK, 0, st>>>(Q.a, Q.b, Q.c, L.a, L.b, L.c, R, rec2, n2, rec_stride, off3, n_rays,
                                                              rays_start, rays_dir, P, alphainv_last, rays_o, rays_d, near, far,
                                                              grad_weights, grad_last, grad_pts, grad_o, grad_d);
  DVGO_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
